// k sparse matrices on ONE pattern: the systems A_t of a Monte-Carlo loop over realizations (Examples 06, 12, 14, 19, 20:
// `for ireal in 1:nreals … pcg(A_t, b_t, 0, Π[p(ξ_t)])`), which differ in numbers only. What they share is held once —
// rowptr, col, the row blocks of spmv_blocks.hpp and their XCD ranges (a CsrDev whose own value array stays empty). What
// differs is one value slab of `capacity` slots, allocated at creation, whose addresses never change:
//
//   slot s = slab + s * stride,   stride = nnz + (nnz mod 2) doubles
//
// The stride is padded to an EVEN count of doubles, so that every slot starts on a 16-byte boundary: the paired loads of
// amg_block_rows read the values as double2 at the even offsets k0 of the row blocks, in every slot as in a CsrOp.
//
// The handle is no operator by itself (usable() is false, as the AMG bank's): mi_op_apply and the single-system solvers
// refuse it before any launch. mi_pcg_batch (batch_solvers.hpp) solves k of its slots in one Krylov loop; the state of
// that loop (BatchWorkspace: kmax state blocks, vectors, partials, residual histories) belongs to the handle, is allocated
// at its first solve and never moves, so the solve graphs captured on it stay valid for the handle's life.
#pragma once
#include "operators.hpp"

namespace mi {

constexpr int BATCH_MAX = 16;            // systems of one batched solve (= AMGB_MAX_TERMS: one term of a bank view each)
constexpr int64_t BATCH_RES_STAGE = 1024; // residual norms per system that travel through pinned memory

// doubles of one slot of a batch on `nnz` stored entries (host arithmetic, no device)
inline int64_t csr_batch_stride(int64_t nnz) { return nnz + (nnz & 1); }

// What the host reads back after a replay of the batched loop (pinned memory, two slots: one replay of run-ahead)
struct BatchFlags {
  long long it[BATCH_MAX];
  int done[BATCH_MAX], overflow[BATCH_MAX];
  int active;   // systems whose stop rule has not fired
  int pad;
};

// The state of one batched Krylov loop: system t at st[t], its vectors at base + t * vs, its partials at base + t * MAX_PARTS,
// its SpMV partials at dot_part + t * dps, its residual norms at res_norm + t * rs.
struct BatchWorkspace {
  int64_t n = 0, vs = 0, dps = 0, rs = 0;
  int g = 1;
  DevBuf<char> slab;
  SolverState *st = nullptr;
  double *part_pAp = nullptr, *part_rr = nullptr, *part_rz = nullptr, *part_bb = nullptr;
  double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *x = nullptr, *b = nullptr;
  double *dot_part = nullptr, *res_norm = nullptr;
  int *sel = nullptr;      // k, then BATCH_MAX slots
  int *active = nullptr;   // systems still iterating (integer atomics)
  BatchFlags *flags = nullptr;   // 2, pinned
  double *res_stage = nullptr;   // BATCH_MAX x BATCH_RES_STAGE, pinned
  hipEvent_t ev[2] = {nullptr, nullptr};

  BatchWorkspace(int64_t n_, int nblocks) : n(n_), g(vec_grid(n_)) {
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    vs = (int64_t)(pad(sizeof(double) * ((size_t)n + 2)) / sizeof(double));
    dps = (int64_t)(pad(sizeof(double) * ((size_t)nblocks + 1)) / sizeof(double));
    rs = (int64_t)(pad(sizeof(double) * ((size_t)n + 2)) / sizeof(double));
    const size_t K = BATCH_MAX;
    const size_t b_st = pad(sizeof(SolverState) * K), b_part = sizeof(double) * MAX_PARTS * K, b_vec = sizeof(double) * (size_t)vs * K;
    const size_t b_dot = sizeof(double) * (size_t)dps * K, b_res = sizeof(double) * (size_t)rs * K, b_sel = pad(sizeof(int) * (K + 2));
    const size_t total = b_st + 4 * b_part + 6 * b_vec + b_dot + b_res + b_sel;
    slab.alloc(total);
    memset_sync(slab.p, 0, total);
    char *q = slab.p;
    st = (SolverState *)q; q += b_st;
    part_pAp = (double *)q; q += b_part; part_rr = (double *)q; q += b_part; part_rz = (double *)q; q += b_part; part_bb = (double *)q; q += b_part;
    r = (double *)q; q += b_vec; z = (double *)q; q += b_vec; p = (double *)q; q += b_vec;
    Ap = (double *)q; q += b_vec; x = (double *)q; q += b_vec; b = (double *)q; q += b_vec;
    dot_part = (double *)q; q += b_dot; res_norm = (double *)q; q += b_res;
    sel = (int *)q; active = sel + K + 1;
    MI_HIP(hipHostMalloc((void **)&flags, 2 * sizeof(BatchFlags)));
    std::memset(flags, 0, 2 * sizeof(BatchFlags));
    MI_HIP(hipHostMalloc((void **)&res_stage, sizeof(double) * K * BATCH_RES_STAGE));
    for (auto &e : ev) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~BatchWorkspace() {
    if (flags) (void)hipHostFree(flags);
    if (res_stage) (void)hipHostFree(res_stage);
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  }
  BatchWorkspace(const BatchWorkspace &) = delete;
  BatchWorkspace &operator=(const BatchWorkspace &) = delete;
};

struct CsrBatchOp : Operator {
  CsrDev A;                 // the pattern; A.val stays empty
  int64_t capacity, nnz, stride;
  DevBuf<double> slab;
  DevBuf<double> stage;     // host-pointer set_values
  std::vector<char> is_set;
  int64_t n_set = 0;
  std::vector<int> rowptr_h, col_h;   // the pattern on the host, for mi_full_assembly_update_batch's one-time comparison
  std::unique_ptr<BatchWorkspace> ws;

  // `h`: the checked pattern (its values are ignored)
  CsrBatchOp(mi_ctx_s *c, HostCsr &h, int64_t capacity_) : Operator(c, h.n_rows), capacity(capacity_), nnz(h.nnz()), stride(csr_batch_stride(h.nnz())) {
    if (h.n_rows != h.n_cols) raise(MI_ERR_BAD_ARG, "mi_csr_batch_create: solver operators must be square");
    h.val.clear();
    A.upload(h, c->stream);
    rowptr_h = h.rowptr; col_h = h.col;
    const double want = 8.0 * (double)stride * (double)capacity;
    if (want >= 9.0e18) raise(MI_ERR_HIP, "mi_csr_batch_create: out of memory: the value slab of %lld slots x %lld bytes asks for %.6g bytes", (long long)capacity,
                              (long long)(8 * stride), want);
    try {
      slab.alloc((size_t)stride * (size_t)capacity);
    } catch (const Error &e) {
      const std::string why = last_error();
      raise(e.code, "mi_csr_batch_create: out of memory: the value slab of %lld slots x %lld bytes asks for %lld bytes: %s", (long long)capacity,
            (long long)(8 * stride), (long long)(8 * stride * capacity), why.c_str());
    }
    is_set.assign((size_t)capacity, 0);
  }
  double *slot(int64_t s) const { return slab.p + (size_t)s * (size_t)stride; }
  void mark_set(int64_t s) { if (!is_set[(size_t)s]) { is_set[(size_t)s] = 1; ++n_set; } }
  BatchWorkspace &workspace() {
    if (!ws) ws.reset(new BatchWorkspace(n, A.nblocks));
    return *ws;
  }
  int64_t bytes_shared() const { return 4 * ((int64_t)n + 1) + 4 * nnz + (int64_t)sizeof(SpmvBlock) * A.nblocks + 4 * 9; }

  bool usable(std::string &why) const override {
    why = "this handle is a batch of sparse matrices (mi_csr_batch_create), which is not applicable itself: solve its slots with mi_pcg_batch";
    return false;
  }
  void apply(const double *, double *, const int *) override {
    std::string why;
    usable(why);
    raise(MI_ERR_BAD_ARG, "%s", why.c_str());
  }
  void bytes(int64_t *a, int64_t *d) const override { *a = 0; *d = 0; }
  void apply_dominant(const double *) override {}
};

}  // namespace mi
