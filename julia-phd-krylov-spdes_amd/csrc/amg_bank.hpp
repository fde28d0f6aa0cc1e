// A bank of smoothed-aggregation hierarchies on ONE symbolic plan: the constant preconditioners of the quantization studies
// (`get_centroidal_preconds`, Example12_…_Functions.jl:85-113; Examples 13, 14, 18, 20), one per centroid, on frozen
// aggregates. What the centroids share is held once — the plan, the index arrays and row blocks of A_l, P_l, R_l, and the
// numeric set-up engine of amg_setup.hpp with its candidate buffers and dense work (an AmgPlanOp that is never applied).
// What differs is numbers only: member p owns slot p of one value slab, allocated at creation, whose addresses never change:
//
//   slot p = [ A_0 .. A_{L-1} | P_0 .. P_{L-2} | R_0 .. R_{L-2} | (ω/d)_0 .. (ω/d)_{L-2} | coarse inverse | (ω_l, g_l) pairs ]
//
// every array padded to an EVEN count of doubles, so that every array of every member starts on a 16-byte boundary: the
// paired loads of amg_block_rows read the values as double2 at even offsets k0 of the row blocks.
//
// set_values(p, val) runs the engine's refresh (the arithmetic of mi_amg_set_values, its kernels unchanged) and only then
// copies the engine's committed buffers into slot p; a refresh that raises MI_ERR_SINGULAR leaves every slot as it was.
// set_values_batch builds k members at once from k slots of a CsrBatch, with the member-indexed kernels and the candidate
// slots of amg_bank_setup.hpp: the same bits, every term committed or kept by itself.
//
// A view (AmgBankView) is the operator: z = Σ_i c_i (Π_{m_i} \ r) for k <= max_terms members, the V(1,1) cycle of amg.hpp for
// all terms in ONE sequence of 4 (L - 1) + 1 launches with the term as the grid's second dimension, then one combination
// launch in the order of k_lincomb. Every kernel reads k and its member index from a small device array and forms its value
// pointers as slab + member * stride + offset, so a captured solve graph serves every later selection; the grid's second
// dimension is max_terms, terms t >= k return at once. The row sums are amg_block_rows and the coarse GEMV order of
// k_amg_coarse, unchanged: a member's cycle has the bits of k_amg_*. No atomics, nothing allocated or synchronised in apply.
//
// apply_batch is the same cycle for k independent right-hand sides, one member each (mi_pcg_batch, batch_solvers.hpp): term t
// reads column t of R and writes column t of Z, and stops under its own flag. Its selection is a device array of its own.
#pragma once
#include "amg_bank_setup.hpp"
#include "vq.hpp"

namespace mi {

constexpr int AMGB_MAX_TERMS = 16;

// sel[0] = k, sel[1 + t] = the member of term t. `stride`: doubles of one slot. Vectors of term t: base + t * (their stride);
// the right-hand side of level 0 is shared (stride 0).
#define MI_AMGB_ARGS int nblocks, const SpmvBlock *__restrict__ blk, const int *__restrict__ rowptr, const int *__restrict__ col, \
                     const double *__restrict__ slab, long long stride, const int *__restrict__ sel
#define MI_AMGB_TERM                                             \
  if (done && *done) return;                                     \
  const int t = (int)blockIdx.y;                                 \
  if (t >= sel[0]) return;                                       \
  const double *slot = slab + (size_t)sel[1 + t] * (size_t)stride; \
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE]

__global__ __launch_bounds__(NT) void k_amgb_down(MI_AMGB_ARGS, long long off_a, long long off_wd, const double *__restrict__ b0, long long bs,
                                                  double *__restrict__ x0, double *__restrict__ r0, long long vs, const int *done) {
  MI_AMGB_TERM;
  const double *val = slot + off_a, *wd = slot + off_wd, *b = b0 + (size_t)t * bs;
  double *x = x0 + (size_t)t * vs, *r = r0 + (size_t)t * vs;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return wd[c] * b[c]; },
                 [&](int i, double s) { const double bi = b[i]; x[i] = wd[i] * bi; r[i] = bi - s; });
}
__global__ __launch_bounds__(NT) void k_amgb_restrict(MI_AMGB_ARGS, long long off_r, const double *__restrict__ v0, long long vs,
                                                      double *__restrict__ y0, long long ys, const int *done) {
  MI_AMGB_TERM;
  const double *val = slot + off_r, *v = v0 + (size_t)t * vs;
  double *y = y0 + (size_t)t * ys;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return v[c]; }, [&](int i, double s) { y[i] = s; });
}
__global__ __launch_bounds__(NT) void k_amgb_prolong(MI_AMGB_ARGS, long long off_p, const double *__restrict__ e0, long long es, double *x0,
                                                     long long vs, const int *done) {
  MI_AMGB_TERM;
  const double *val = slot + off_p, *e = e0 + (size_t)t * es;
  double *x = x0 + (size_t)t * vs;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return e[c]; }, [&](int i, double s) { x[i] = x[i] + s; });
}
__global__ __launch_bounds__(NT) void k_amgb_post(MI_AMGB_ARGS, long long off_a, long long off_wd, const double *__restrict__ b0, long long bs,
                                                  const double *__restrict__ x0, long long vs, double *__restrict__ y0, long long ys,
                                                  const int *done) {
  MI_AMGB_TERM;
  const double *val = slot + off_a, *wd = slot + off_wd, *b = b0 + (size_t)t * bs, *x = x0 + (size_t)t * vs;
  double *y = y0 + (size_t)t * ys;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return x[c]; },
                 [&](int i, double s) { y[i] = x[i] + wd[i] * (b[i] - s); });
}
#undef MI_AMGB_TERM
// The batched cycle (AmgBankView::apply_batch): term t is system t of a batched solve, Z[:, t] = Π_{member t} \ R[:, t]. The same
// row sums; `sel` is the view's BATCH selection, the stop flag is per term (done[t * ds], ds in ints), and the level-0
// right-hand side has a stride of its own. The last launch stores 0.0 + 1.0 * z, the arithmetic of k_amgb_combine for one term
// with coefficient 1: a system's cycle has the bits of view.select(member) applied to its column.
#define MI_AMGBB_TERM                                            \
  const int t = (int)blockIdx.y;                                 \
  if (t >= sel[0]) return;                                       \
  if (done && done[(size_t)t * (size_t)ds]) return;              \
  const double *slot = slab + (size_t)sel[1 + t] * (size_t)stride; \
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE]
__global__ __launch_bounds__(NT) void k_amgbb_down(MI_AMGB_ARGS, long long off_a, long long off_wd, const double *__restrict__ b0, long long bs,
                                                   double *__restrict__ x0, double *__restrict__ r0, long long vs, const int *done, long long ds) {
  MI_AMGBB_TERM;
  const double *val = slot + off_a, *wd = slot + off_wd, *b = b0 + (size_t)t * bs;
  double *x = x0 + (size_t)t * vs, *r = r0 + (size_t)t * vs;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return wd[c] * b[c]; },
                 [&](int i, double s) { const double bi = b[i]; x[i] = wd[i] * bi; r[i] = bi - s; });
}
__global__ __launch_bounds__(NT) void k_amgbb_restrict(MI_AMGB_ARGS, long long off_r, const double *__restrict__ v0, long long vs,
                                                       double *__restrict__ y0, long long ys, const int *done, long long ds) {
  MI_AMGBB_TERM;
  const double *val = slot + off_r, *v = v0 + (size_t)t * vs;
  double *y = y0 + (size_t)t * ys;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return v[c]; }, [&](int i, double s) { y[i] = s; });
}
__global__ __launch_bounds__(NT) void k_amgbb_prolong(MI_AMGB_ARGS, long long off_p, const double *__restrict__ e0, long long es, double *x0,
                                                      long long vs, const int *done, long long ds) {
  MI_AMGBB_TERM;
  const double *val = slot + off_p, *e = e0 + (size_t)t * es;
  double *x = x0 + (size_t)t * vs;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return e[c]; }, [&](int i, double s) { x[i] = x[i] + s; });
}
// fin: this is the cycle's last launch (level 0)
__global__ __launch_bounds__(NT) void k_amgbb_post(MI_AMGB_ARGS, long long off_a, long long off_wd, const double *__restrict__ b0, long long bs,
                                                   const double *__restrict__ x0, long long vs, double *__restrict__ y0, long long ys, int fin,
                                                   const int *done, long long ds) {
  MI_AMGBB_TERM;
  const double *val = slot + off_a, *wd = slot + off_wd, *b = b0 + (size_t)t * bs, *x = x0 + (size_t)t * vs;
  double *y = y0 + (size_t)t * ys;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return x[c]; }, [&](int i, double s) {
    const double v = x[i] + wd[i] * (b[i] - s);
    y[i] = fin ? 0.0 + 1.0 * v : v;
  });
}
#undef MI_AMGBB_TERM
#undef MI_AMGB_ARGS
// y_t = Z_{m_t} b_t, the order of k_amg_coarse; fin: a coarse-only cycle, this is its last launch
__global__ __launch_bounds__(NT) void k_amgbb_coarse(int n, const double *__restrict__ slab, long long stride, const int *__restrict__ sel,
                                                     long long off_z, const double *__restrict__ b0, long long bs, double *__restrict__ y0,
                                                     long long ys, int fin, const int *done, long long ds) {
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  if (done && done[(size_t)t * (size_t)ds]) return;
  const int row = (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double *z = slab + (size_t)sel[1 + t] * (size_t)stride + off_z + (size_t)row * n;
  const double *b = b0 + (size_t)t * bs;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += z[j] * b[j];
  s = wave_sum(s);
  if (lane == 0) y0[(size_t)t * ys + row] = fin ? 0.0 + 1.0 * s : s;
}
// y_t = Z_{m_t} b_t: one wave per row, the order of k_amg_coarse
__global__ __launch_bounds__(NT) void k_amgb_coarse(int n, const double *__restrict__ slab, long long stride, const int *__restrict__ sel,
                                                    long long off_z, const double *__restrict__ b0, long long bs, double *__restrict__ y0,
                                                    long long ys, const int *done) {
  if (done && *done) return;
  const int t = (int)blockIdx.y;
  if (t >= sel[0]) return;
  const int row = (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double *z = slab + (size_t)sel[1 + t] * (size_t)stride + off_z + (size_t)row * n;
  const double *b = b0 + (size_t)t * bs;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += z[j] * b[j];
  s = wave_sum(s);
  if (lane == 0) y0[(size_t)t * ys + row] = s;
}
// z = Σ_{i < k} c[i] * t_i, i ascending from +0 (product, then sum): k_lincomb with k read on the device
__global__ __launch_bounds__(NT) void k_amgb_combine(int n, const int *__restrict__ sel, const double *__restrict__ coef,
                                                     const double *__restrict__ T, double *__restrict__ z, const int *done) {
  if (done && *done) return;
  const int k = sel[0];
  for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
    double acc = 0.0;
    for (int i = 0; i < k; ++i) acc = acc + coef[i] * T[(size_t)i * n + e];
    z[e] = acc;
  }
}

// ------------------------------------------------------------------ the bank (not applicable itself)
struct AmgBankOp : Operator {
  AmgPlanOp eng;                       // plan, index arrays and row blocks, candidates, dense work; its own buffers stage a member
  int64_t capacity;
  int nlev, nc;
  std::vector<int64_t> off_a, off_p, off_r, off_wd;   // doubles from the start of a slot
  int64_t off_z = 0, off_om = 0, stride = 0, padding = 0;   // doubles; padding: the doubles added to make every count even
  DevBuf<double> slab;
  std::vector<char> is_set;
  std::vector<double> omega_h;         // capacity x (L - 1): ω_l of every member, for the read-back
  int64_t n_set = 0;
  int views = 0;

  static int64_t even(int64_t cnt, int64_t &pad) { pad += cnt & 1; return cnt + (cnt & 1); }

  AmgBankOp(mi_ctx_s *c, int64_t n0, const int64_t *rowptr, const int64_t *colidx, int64_t nlevels, const int64_t *n_l,
            const int64_t *const *agg, int64_t capacity_, int base)
      : Operator(c, n0), eng(c, n0, rowptr, colidx, nullptr, nlevels, n_l, agg, base), capacity(capacity_) {
    nlev = eng.nlev; nc = eng.nc;
    const size_t L = (size_t)nlev;
    off_a.resize(L); off_p.resize(L - 1); off_r.resize(L - 1); off_wd.resize(L - 1);
    int64_t at = 0;
    for (size_t l = 0; l < L; ++l) { off_a[l] = at; at += even(eng.plan.lv[l].a_nnz(), padding); }
    for (size_t l = 0; l + 1 < L; ++l) { off_p[l] = at; at += even(eng.plan.lv[l].p_nnz(), padding); }
    for (size_t l = 0; l + 1 < L; ++l) { off_r[l] = at; at += even(eng.plan.lv[l].p_nnz(), padding); }
    for (size_t l = 0; l + 1 < L; ++l) { off_wd[l] = at; at += even(eng.plan.lv[l].n, padding); }
    off_z = at; at += even((int64_t)nc * nc, padding);
    off_om = at; at += 2 * ((int64_t)L - 1);
    stride = at;
    const double want = 8.0 * (double)stride * (double)capacity;
    if (want >= 9.0e18) raise(MI_ERR_HIP, "mi_amg_bank_create: out of memory: the value slab of %lld members x %lld bytes asks for %.6g bytes", (long long)capacity,
                              (long long)(8 * stride), want);
    try {
      slab.alloc((size_t)stride * (size_t)capacity);
    } catch (const Error &e) {
      const std::string why = last_error();
      raise(e.code, "mi_amg_bank_create: out of memory: the value slab of %lld members x %lld bytes asks for %lld bytes: %s", (long long)capacity,
            (long long)(8 * stride), (long long)(8 * stride * capacity), why.c_str());
    }
    is_set.assign((size_t)capacity, 0);
    omega_h.assign((size_t)capacity * std::max<size_t>(1, L - 1), 0.0);
  }

  double *slot(int64_t m) const { return slab.p + (size_t)m * (size_t)stride; }

  // the numeric chain on the device values `a0`; committed into slot `m` only when it succeeds. Synchronous.
  void set_values(int64_t m, const double *a0) {
    eng.refresh(a0, "mi_amg_bank_set_values");   // raises MI_ERR_SINGULAR: no slot is touched
    hipStream_t s = ctx->stream;
    double *d = slot(m);
    auto copy = [&](int64_t off, const double *src, int64_t cnt) {
      if (cnt) MI_HIP(hipMemcpyAsync(d + off, src, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, s));
    };
    for (int l = 0; l < nlev; ++l) {
      const amgp::Level &H = eng.plan.lv[(size_t)l];
      AmgOp::Level &L = eng.lv[(size_t)l];
      copy(off_a[(size_t)l], L.A.val.p, H.a_nnz());
      if (l == nlev - 1) break;
      copy(off_p[(size_t)l], L.P.val.p, H.p_nnz()); copy(off_r[(size_t)l], L.R.val.p, H.p_nnz()); copy(off_wd[(size_t)l], L.wd.p, H.n);
    }
    copy(off_z, eng.zinv.p, (int64_t)nc * nc);
    copy(off_om, eng.om.p, 2 * ((int64_t)nlev - 1));
    MI_HIP(hipStreamSynchronize(s));
    for (int l = 0; l + 1 < nlev; ++l) omega_h[(size_t)m * (size_t)(nlev - 1) + (size_t)l] = eng.omega_h[(size_t)l];
    if (!is_set[(size_t)m]) { is_set[(size_t)m] = 1; ++n_set; }
  }

  // Members members[t] from the device values a_slab + slots[t] * a_stride, t < k, in one sequence of launches
  // (amg_bank_setup.hpp). Every healthy term is committed — A_0 from where it lies, then one copy of its candidate slot —
  // and a failed one leaves its member as it was; term[t] says which. Synchronous. The caller has checked k, the members
  // (distinct, in range) and the slots.
  AmgBankSetupWs bws;
  unsigned long long batch_serial = 0; // Operator::serial of the CsrBatch whose pattern was compared with this bank's in full (0: none)
  void set_values_batch(int k, const int64_t *members, const int64_t *slots, const double *a_slab, int64_t a_stride, std::vector<AsbTerm> &term) {
    const int64_t a0_len = nlev > 1 ? off_a[1] : off_z;
    amg_bank_setup_batch(eng, bws, k, members, slots, a_slab, a_stride, off_a, off_p, off_r, off_wd, off_z, off_om, stride, a0_len, term);
    hipStream_t s = ctx->stream;
    const size_t nom = 2 * (size_t)(nlev - 1);
    std::vector<double> oh((size_t)k * std::max<size_t>(1, nom));
    for (int t = 0; t < k; ++t) {
      if (!term[(size_t)t].ok) continue;
      double *d = slot(members[t]);
      const double *c = bws.cand.p + (size_t)t * (size_t)bws.cs;
      if (eng.nnz0) MI_HIP(hipMemcpyAsync(d, a_slab + (size_t)slots[t] * (size_t)a_stride, (size_t)eng.nnz0 * sizeof(double), hipMemcpyDeviceToDevice, s));
      MI_HIP(hipMemcpyAsync(d + a0_len, c, (size_t)bws.cs * sizeof(double), hipMemcpyDeviceToDevice, s));
      if (nom) MI_HIP(hipMemcpyAsync(oh.data() + (size_t)t * nom, c + (off_om - a0_len), nom * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    MI_HIP(hipStreamSynchronize(s));
    for (int t = 0; t < k; ++t) {
      if (!term[(size_t)t].ok) continue;
      const size_t m = (size_t)members[t];
      for (int l = 0; l + 1 < nlev; ++l) omega_h[m * (size_t)(nlev - 1) + (size_t)l] = oh[(size_t)t * nom + (size_t)2 * l];
      if (!is_set[m]) { is_set[m] = 1; ++n_set; }
    }
  }

  // read-back of one level of member `m`, as AmgOp::level_get (HOST arrays, 0-based, any pointer may be NULL)
  void level_get(int64_t m, int l, int64_t *a_ptr, int64_t *a_col, double *a_val, int64_t *p_ptr, int64_t *p_col, double *p_val, double *omega,
                 double *wd_out) {
    hipStream_t s = ctx->stream;
    AmgOp::Level &L = eng.lv[(size_t)l];
    const double *d = slot(m);
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
    ints(L.A.rowptr.p, (size_t)L.A.n_rows + 1, a_ptr); ints(L.A.col.p, (size_t)L.A.nnz, a_col); vals(d + off_a[(size_t)l], (size_t)L.A.nnz, a_val);
    if (l == nlev - 1) return;
    ints(L.P.rowptr.p, (size_t)L.P.n_rows + 1, p_ptr); ints(L.P.col.p, (size_t)L.P.nnz, p_col); vals(d + off_p[(size_t)l], (size_t)L.P.nnz, p_val);
    if (omega) *omega = omega_h[(size_t)m * (size_t)(nlev - 1) + (size_t)l];
    vals(d + off_wd[(size_t)l], (size_t)L.n, wd_out);
  }

  bool usable(std::string &why) const override {
    why = "this handle is an AMG bank (mi_amg_bank_create), which is not applicable itself: apply and solve with a view of it (mi_amg_bank_view)";
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

// ------------------------------------------------------------------ a view: the operator z = Σ_i c_i (Π_{m_i} \ r)
struct AmgBankView : Operator {
  AmgBankOp *bank;
  int kmax;
  DevBuf<int> sel;                 // k, then kmax member indices
  DevBuf<double> coef;             // kmax
  struct Vec { DevBuf<double> b, x, r, y; int64_t vs = 0; };   // level vectors of kmax terms, term t at t * vs
  std::vector<Vec> lv;
  DevBuf<double> tmp;              // kmax x n: the terms' results
  std::vector<int64_t> sel_h;      // the selection, on the host
  DevBuf<int> bsel;                // apply_batch: k, then kmax member indices; written by the batched solve's entry kernel

  AmgBankView(mi_ctx_s *c, AmgBankOp *b, int max_terms) : Operator(c, b->n), bank(b), kmax(max_terms) {
    sel.alloc((size_t)kmax + 1); coef.alloc((size_t)kmax);
    bsel.alloc((size_t)kmax + 1);
    memset_sync(bsel.p, 0, ((size_t)kmax + 1) * sizeof(int));
    const int L = bank->nlev;
    lv.resize((size_t)L);
    for (int l = 0; l < L; ++l) {
      Vec &V = lv[(size_t)l];
      V.vs = (int64_t)bank->eng.lv[(size_t)l].n + 1;
      const size_t m = (size_t)V.vs * (size_t)kmax;
      if (l > 0) { V.b.alloc(m); V.y.alloc(m); }
      if (l < L - 1) { V.x.alloc(m); V.r.alloc(m); }
    }
    tmp.alloc((size_t)kmax * (size_t)n);
    const int64_t m0 = 0;
    const double one = 1.0;
    write_selection(1, &m0, &one);
    ++bank->views;   // last: nothing above may leave a count behind
  }
  ~AmgBankView() override { --bank->views; }

  // a blocking copy on the context's stream, as CombineOp::set_coefficients: ordered after the solves already enqueued
  void write_selection(int64_t k, const int64_t *members, const double *cf) {
    std::vector<int> s((size_t)kmax + 1, 0);
    std::vector<double> cc((size_t)kmax, 0.0);
    s[0] = (int)k;
    for (int64_t i = 0; i < k; ++i) { s[(size_t)i + 1] = (int)members[i]; cc[(size_t)i] = cf[i]; }
    MI_HIP(hipMemcpyAsync(sel.p, s.data(), s.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipMemcpyAsync(coef.p, cc.data(), cc.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    sel_h.assign(members, members + k);
  }

  bool usable(std::string &why) const override {
    for (int64_t m : sel_h)
      if (!bank->is_set[(size_t)m]) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "the view selects member %lld of the AMG bank, which was never set (mi_amg_bank_set_values)", (long long)m);
        why = buf;
        return false;
      }
    return true;
  }

  static int grid_of(const CsrDev &M) { return ((M.nblocks + 7) / 8) * 8; }
#define MI_AMGB_CSR(M) (M).nblocks, (const SpmvBlock *)(M).blk.p, (const int *)(M).rowptr.p, (const int *)(M).col.p, (const double *)bank->slab.p, \
                       (long long)bank->stride, (const int *)sel.p
  void coarse(const double *b, long long bs, double *y, long long ys, const int *done) {
    const int nc = bank->nc;
    hipLaunchKernelGGL(k_amgb_coarse, dim3((nc + NT / 64 - 1) / (NT / 64), kmax), dim3(NT), 0, ctx->stream, nc, (const double *)bank->slab.p,
                       (long long)bank->stride, (const int *)sel.p, (long long)bank->off_z, b, bs, y, ys, done);
  }
  void combine(double *z, const int *done) {
    hipLaunchKernelGGL(k_amgb_combine, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, (int)n, (const int *)sel.p, (const double *)coef.p,
                       (const double *)tmp.p, z, done);
    MI_HIP(hipGetLastError());
  }
  void apply(const double *r, double *z, const int *done) override {
    std::string why;
    if (!usable(why)) raise(MI_ERR_BAD_ARG, "%s", why.c_str());
    hipStream_t s = ctx->stream;
    const int L = bank->nlev;
    const unsigned ky = (unsigned)kmax;
    if (L == 1) { coarse(r, 0, tmp.p, (long long)n, done); combine(z, done); return; }
    for (int l = 0; l < L - 1; ++l) {
      AmgOp::Level &E = bank->eng.lv[(size_t)l];
      Vec &V = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? V.b.p : r;
      const long long bs = l ? V.vs : 0;
      hipLaunchKernelGGL(k_amgb_down, dim3(grid_of(E.A), ky), dim3(NT), 0, s, MI_AMGB_CSR(E.A), (long long)bank->off_a[(size_t)l],
                         (long long)bank->off_wd[(size_t)l], b, bs, V.x.p, V.r.p, (long long)V.vs, done);
      hipLaunchKernelGGL(k_amgb_restrict, dim3(grid_of(E.R), ky), dim3(NT), 0, s, MI_AMGB_CSR(E.R), (long long)bank->off_r[(size_t)l],
                         (const double *)V.r.p, (long long)V.vs, N.b.p, (long long)N.vs, done);
    }
    Vec &C = lv[(size_t)L - 1];
    coarse(C.b.p, C.vs, C.y.p, C.vs, done);
    for (int l = L - 2; l >= 0; --l) {
      AmgOp::Level &E = bank->eng.lv[(size_t)l];
      Vec &V = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? V.b.p : r;
      const long long bs = l ? V.vs : 0;
      hipLaunchKernelGGL(k_amgb_prolong, dim3(grid_of(E.P), ky), dim3(NT), 0, s, MI_AMGB_CSR(E.P), (long long)bank->off_p[(size_t)l],
                         (const double *)N.y.p, (long long)N.vs, V.x.p, (long long)V.vs, done);
      hipLaunchKernelGGL(k_amgb_post, dim3(grid_of(E.A), ky), dim3(NT), 0, s, MI_AMGB_CSR(E.A), (long long)bank->off_a[(size_t)l],
                         (long long)bank->off_wd[(size_t)l], b, bs, (const double *)V.x.p, (long long)V.vs, l ? V.y.p : tmp.p,
                         l ? (long long)V.vs : (long long)n, done);
    }
    combine(z, done);
  }
  // Z[:, t] = Π_{bsel[1 + t]} \ R[:, t] for t < bsel[0] (column strides ldr, ldz): the launches of apply() with the term as the
  // system, no combination launch, every term under its own stop flag done[t * ds] (done == NULL: none). The caller has
  // checked that the members are set and has written bsel on this stream; select / combine state is not touched.
  void apply_batch(const double *R, long long ldr, double *Z, long long ldz, const int *done, long long ds) {
    hipStream_t s = ctx->stream;
    const int L = bank->nlev;
    const unsigned ky = (unsigned)kmax;
    const int nc = bank->nc;
    auto coarse_b = [&](const double *b, long long bs, double *y, long long ys, int fin) {
      hipLaunchKernelGGL(k_amgbb_coarse, dim3((nc + NT / 64 - 1) / (NT / 64), ky), dim3(NT), 0, s, nc, (const double *)bank->slab.p,
                         (long long)bank->stride, (const int *)bsel.p, (long long)bank->off_z, b, bs, y, ys, fin, done, ds);
    };
#define MI_AMGBB_CSR(M) (M).nblocks, (const SpmvBlock *)(M).blk.p, (const int *)(M).rowptr.p, (const int *)(M).col.p, (const double *)bank->slab.p, \
                        (long long)bank->stride, (const int *)bsel.p
    if (L == 1) { coarse_b(R, ldr, Z, ldz, 1); MI_HIP(hipGetLastError()); return; }
    for (int l = 0; l < L - 1; ++l) {
      AmgOp::Level &E = bank->eng.lv[(size_t)l];
      Vec &V = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? V.b.p : R;
      const long long bs = l ? V.vs : ldr;
      hipLaunchKernelGGL(k_amgbb_down, dim3(grid_of(E.A), ky), dim3(NT), 0, s, MI_AMGBB_CSR(E.A), (long long)bank->off_a[(size_t)l],
                         (long long)bank->off_wd[(size_t)l], b, bs, V.x.p, V.r.p, (long long)V.vs, done, ds);
      hipLaunchKernelGGL(k_amgbb_restrict, dim3(grid_of(E.R), ky), dim3(NT), 0, s, MI_AMGBB_CSR(E.R), (long long)bank->off_r[(size_t)l],
                         (const double *)V.r.p, (long long)V.vs, N.b.p, (long long)N.vs, done, ds);
    }
    Vec &C = lv[(size_t)L - 1];
    coarse_b(C.b.p, C.vs, C.y.p, C.vs, 0);
    for (int l = L - 2; l >= 0; --l) {
      AmgOp::Level &E = bank->eng.lv[(size_t)l];
      Vec &V = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? V.b.p : R;
      const long long bs = l ? V.vs : ldr;
      hipLaunchKernelGGL(k_amgbb_prolong, dim3(grid_of(E.P), ky), dim3(NT), 0, s, MI_AMGBB_CSR(E.P), (long long)bank->off_p[(size_t)l],
                         (const double *)N.y.p, (long long)N.vs, V.x.p, (long long)V.vs, done, ds);
      hipLaunchKernelGGL(k_amgbb_post, dim3(grid_of(E.A), ky), dim3(NT), 0, s, MI_AMGBB_CSR(E.A), (long long)bank->off_a[(size_t)l],
                         (long long)bank->off_wd[(size_t)l], b, bs, (const double *)V.x.p, (long long)V.vs, l ? V.y.p : Z,
                         l ? (long long)V.vs : ldz, l ? 0 : 1, done, ds);
    }
#undef MI_AMGBB_CSR
    MI_HIP(hipGetLastError());
  }
  // k cycles (AmgOp::bytes each) and the combination; dominant: the fine-level k_amgb_down of the terms selected
  void bytes(int64_t *a, int64_t *d) const override {
    const int64_t k = (int64_t)sel_h.size();
    *a = k * bank->eng.alg + 8 * n * (k + 1);
    *d = k * bank->eng.dom;
  }
  void apply_dominant(const double *x) override {
    std::string why;
    if (!usable(why)) raise(MI_ERR_BAD_ARG, "%s", why.c_str());
    if (bank->nlev == 1) { coarse(x, 0, tmp.p, (long long)n, nullptr); return; }
    AmgOp::Level &E = bank->eng.lv[0];
    Vec &V = lv[0];
    hipLaunchKernelGGL(k_amgb_down, dim3(grid_of(E.A), (unsigned)kmax), dim3(NT), 0, ctx->stream, MI_AMGB_CSR(E.A), (long long)bank->off_a[0],
                       (long long)bank->off_wd[0], x, 0ll, V.x.p, V.r.p, (long long)V.vs, (const int *)nullptr);
  }
#undef MI_AMGB_CSR
};

}  // namespace mi
