// `Pl` = smoothed-aggregation AMG inside the device interior CG (mi_schur_interior_amg): the reference's
// `IterativeSolvers.cg(A_IId, rhs; Pl = Π_IId, reltol)` of apply_local_schur(s), apply_global_schur, get_schur_rhs and
// get_subdomain_solutions (EPDD.jl:609-619, 648-650, 813-815, 1021) with Π_IId an AMG preconditioner (Example07:174).
//
// ONE hierarchy of the stacked block-diagonal A_II = blockdiag(A_IIdd) of the operator's subdomains, built by the plan
// machinery of amg_plan.hpp / amg_setup.hpp on the operator's own pattern and current values: ω_l is the Gershgorin maximum
// over all subdomains, the stop rule counts stacked rows, the coarsest level has one dense inverse. Every level is block
// diagonal (an aggregate that holds nodes of two subdomains is refused), so M is a block-diagonal SPD operator and the
// subdomains' CG iterations stay independent; the coarsest GEMV keeps to the columns of the row's own subdomain
// (k_amg_coarse_dom), so that a right-hand side that is not finite in one subdomain does not reach the others.
// The loop: operators.hpp InteriorCg (pl == ICG_PL_EXT), the EXT instantiations of kernels.hpp's k_icg_init / k_icg_start /
// k_icg_update / k_icg_direction<IcgPl>. The partials of r'z come from the level-0 post-smoothing
// launch (k_amg_post_dot) on row blocks cut at the subdomain boundaries — the row blocks of the interior CG's own SpMV.
#pragma once
#include "amg_setup.hpp"

namespace mi {

struct InteriorAmgStats { int64_t levels, coarse_n, bytes_kept; };

inline void interior_amg_select(mi_ctx_s *c, InteriorCg &icg, int64_t nlevels, const int64_t *n_l, const int64_t *const *agg, int base) {
  const char *me = "mi_schur_interior_amg";
  if (c->n_ranks > 1 || c->has_comm()) raise(MI_ERR_BAD_ARG, "%s: the hierarchy is built on one device only; this context has a communicator", me);
  if (base != 0 && base != 1) raise(MI_ERR_BAD_ARG, "%s: index_base = %d (0 or 1)", me, base);
  if (!n_l) raise(MI_ERR_BAD_ARG, "%s: n_l is NULL", me);
  hipStream_t s = c->stream;
  const int n = icg.n, ndl = icg.ndl;
  if (n < 1) raise(MI_ERR_BAD_ARG, "%s: the operator has no interior unknowns", me);
  // the stacked A_II as the interior CG holds it
  const size_t nnz = (size_t)icg.A.nnz;
  std::vector<int> rp((size_t)n + 1), ci(nnz);
  std::vector<double> val(nnz);
  MI_HIP(hipStreamSynchronize(s));
  memcpy_sync(rp.data(), icg.A.rowptr.p, sizeof(int) * rp.size(), hipMemcpyDeviceToHost);
  if (nnz) {
    memcpy_sync(ci.data(), icg.A.col.p, sizeof(int) * nnz, hipMemcpyDeviceToHost);
    memcpy_sync(val.data(), icg.A.val.p, sizeof(double) * nnz, hipMemcpyDeviceToHost);
  }
  std::vector<int64_t> rp64(rp.size()), ci64(nnz);
  for (size_t i = 0; i < rp.size(); ++i) rp64[i] = (int64_t)rp[i] + base;
  for (size_t k = 0; k < nnz; ++k) ci64[k] = (int64_t)ci[k] + base;
  std::vector<int> breaks(icg.ioff_h.begin(), icg.ioff_h.end());
  std::unique_ptr<AmgPlanOp> P;
  try {
    P.reset(new AmgPlanOp(c, n, rp64.data(), ci64.data(), val.data(), nlevels, n_l, agg, base, &breaks));
  } catch (const Error &e) {
    const std::string why = last_error();
    raise(e.code, "%s: the stacked A_II (%d rows, %d subdomains): %s", me, n, ndl, why.c_str());
  }
  // the subdomain of every node, level by level
  std::vector<int> dom((size_t)n);
  for (int d = 0; d < ndl; ++d) {
    const int hi = d + 1 < ndl ? icg.ioff_h[(size_t)d + 1] : n;
    for (int i = icg.ioff_h[(size_t)d]; i < hi; ++i) dom[(size_t)i] = d;
  }
  for (int l = 0; l + 1 < P->nlev; ++l) {
    const amgp::Level &H = P->plan.lv[(size_t)l];
    std::vector<int> nxt((size_t)H.nc, -1);
    for (int i = 0; i < H.n; ++i) {
      int &t = nxt[(size_t)H.agg[(size_t)i]];
      if (t < 0) t = dom[(size_t)i];
      else if (t != dom[(size_t)i])
        raise(MI_ERR_BAD_ARG, "%s: level %d: aggregate %d holds nodes of the subdomains %d and %d; the hierarchy has to be block diagonal", me, l,
              H.agg[(size_t)i], t, dom[(size_t)i]);
    }
    dom.swap(nxt);
  }
  P->coarse_dom.upload(dom, s);
  // where the partials of r'z of every subdomain lie
  std::vector<int> q0((size_t)ndl, 0), q1((size_t)ndl, 0);
  size_t nparts;
  if (P->nlev == 1) {
    nparts = (size_t)n;
    for (int d = 0; d < ndl; ++d) { q0[(size_t)d] = icg.ioff_h[(size_t)d]; q1[(size_t)d] = d + 1 < ndl ? icg.ioff_h[(size_t)d + 1] : n; }
  } else {
    const std::vector<SpmvBlock> &B = P->lv[0].A.blocks_h;
    nparts = B.size();
    int d = 0;
    std::vector<char> seen((size_t)ndl, 0);
    for (int b = 0; b < (int)B.size(); ++b) {
      while (d + 1 < ndl && B[(size_t)b].r0 >= icg.ioff_h[(size_t)d + 1]) ++d;
      const int hi = d + 1 < ndl ? icg.ioff_h[(size_t)d + 1] : n;
      if (B[(size_t)b].r1 > hi) raise(MI_ERR_BAD_ARG, "%s: row block %d crosses the boundary of subdomain %d", me, b, d);
      if (!seen[(size_t)d]) { seen[(size_t)d] = 1; q0[(size_t)d] = b; }
      q1[(size_t)d] = b + 1;
    }
  }
  AmgPlanOp *raw = P.get();
  IcgExtPl e;
  e.op = std::move(P);
  e.cycle = [raw](const double *r, double *z, double *part, const int *done) { raw->cycle(r, z, done, part); };
  e.refresh = [raw](const double *a0) { raw->refresh(a0, "mi_schur_matfree_set_values"); };
  e.q0 = std::move(q0); e.q1 = std::move(q1); e.nparts = nparts;
  icg.select(ICG_PL_EXT, std::move(e));
}

inline bool interior_amg_stats(const InteriorCg &icg, InteriorAmgStats *st) {
  const AmgPlanOp *P = icg.pl == ICG_PL_EXT ? dynamic_cast<const AmgPlanOp *>(icg.ext.op.get()) : nullptr;
  if (!P) return false;
  st->levels = P->nlev; st->coarse_n = P->nc;
  st->bytes_kept = P->kept + 8 * (int64_t)(icg.zv.n + icg.p_rzq.n) + 4 * (int64_t)(P->coarse_dom.n + icg.dom_q0.n + icg.dom_q1.n);
  return true;
}

}  // namespace mi
