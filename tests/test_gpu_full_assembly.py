"""GPU suite (-m gpu): the full-system assembly on the device and the in-place refresh of A, b and the Jacobi M.

All comparisons are BITWISE (`np.array_equal` on the values and on their sign bits): the device kernel does the operations of
`fem.do_isotropic_elliptic_assembly` in the same order, and an operator refreshed in place holds the values of a fresh one.

  * `api.FullAssemblyPlan.run` equals the host assembly for numpy and for torch input on every mesh of the CPU test and on
    N = 60; it equals `api.AssemblyPlan(ctx, plan.as_block_plan()).run(a)`; it repeats itself, also after another coefficient;
  * `A_op.set_values` / `FullAssemblyPlan.update`: `A_op * x`, and `pcg` after graphs were captured on the old values, have the
    bits of a fresh operator's; `JacobiPreconditioner.refresh(A_op)` equals a new `JacobiPreconditioner(A.diagonal())`;
  * the loop of Example06 with device tensors only, two realizations, against the host-assembled flow;
  * refusals raise MiError and leave operator and plan usable."""
import ctypes as C

import numpy as np
import pytest

import full_assembly_cases as cases
from conftest import f_m1, lognormal_coeff, u0734

pytestmark = pytest.mark.gpu

MESHES = [f"grid{N}" for N in cases.GRID_SIZES] + ["grid60", "unstructured", "fan40", "fan4095"]


@pytest.fixture(scope="module")
def meshes(fem):
    assert fem.FA_SEG - 1 == 4095
    return cases.mesh_cases(fem, fans=(40, fem.FA_SEG - 1), grids=cases.GRID_SIZES + (60,))


@pytest.fixture(scope="module")
def grid60(fem):
    """N = 60 with Example06's f and uexact: the mesh, the plan and the host systems of three coefficients"""
    mesh = fem.get_mesh(60)
    plan = cases.make_plan(fem, mesh, f_m1, u0734)
    coeffs = [np.ones(mesh.points.shape[1])] + [lognormal_coeff(fem, mesh.points, s) for s in (1, 2)]
    systems = [cases.host_system(fem, mesh, a, f_m1, u0734)[1:] for a in coeffs]
    return mesh, plan, coeffs, systems


@pytest.mark.parametrize("name", MESHES)
def test_device_run_has_the_bits_of_the_host_assembly(pkg, ctx, fem, meshes, name):
    import torch
    mesh = meshes[name]
    for label, a, f, uexact in cases.runs(fem, mesh):
        _, A, b = cases.host_system(fem, mesh, a, f, uexact)
        plan = cases.make_plan(fem, mesh, f, uexact)
        dev = pkg.api.FullAssemblyPlan(ctx, plan)
        vals, rhs = dev.run(a)
        assert cases.same_bits(vals, A.data) and cases.same_bits(rhs, b), (name, label)
        vt, bt = dev.run(torch.from_numpy(a).cuda())
        ctx.synchronize()                                    # device-pointer calls are asynchronous on the context's stream
        assert vt.is_cuda and bt.is_cuda and cases.same_bits(vt.cpu().numpy(), A.data) and cases.same_bits(bt.cpu().numpy(), b)
        generic = pkg.api.AssemblyPlan(ctx, plan.as_block_plan())
        out = generic.run(a)
        assert cases.same_bits(out[:plan.nnz], vals) and cases.same_bits(out[plan.nnz:], rhs), (name, label)
        # a second run; another coefficient in between; the 1-based ABI
        other = 1.0 + np.arange(a.size) / a.size
        v2, b2 = dev.run(a)
        vo, bo = dev.run(other)
        v3, b3 = dev.run(a)
        assert cases.same_bits(v2, vals) and cases.same_bits(b2, rhs) and cases.same_bits(v3, vals) and cases.same_bits(b3, rhs)
        _, Ao, bo_h = cases.host_system(fem, mesh, other, f, uexact)
        assert cases.same_bits(vo, Ao.data) and cases.same_bits(bo, bo_h) and not np.array_equal(vo, vals)
        if label == "constant":
            one_based = pkg.api.FullAssemblyPlan(ctx, plan, index_base=1)
            v1, b1 = one_based.run(a)
            assert cases.same_bits(v1, vals) and cases.same_bits(b1, rhs)
            one_based.close()
        st = dev.stats()
        assert st == dict(row_blocks=plan.blk_row.size - 1, incidences=plan.inc_code.size, bytes_kept=plan.bytes())
        generic.close()
        dev.close()


def test_set_values_update_and_jacobi_refresh(pkg, ctx, fem, grid60):
    import torch
    api = pkg.api
    mesh, plan, (a0, a1, a2), ((A0, b0), (A1, b1), (A2, b2)) = grid60
    n = plan.n
    dev = api.FullAssemblyPlan(ctx, plan)
    x = np.random.default_rng(0).standard_normal(n)
    x0 = np.zeros(n)
    A_op = api.SparseMatrixCSC(ctx, A0)
    assert isinstance(A_op, api.Operator)
    M = api.JacobiPreconditioner(ctx, A0.diagonal())
    before = api.pcg(A_op, b0, x0, M)                                   # graphs are captured on the old values
    fresh1, fresh2 = api.SparseMatrixCSC(ctx, A1), api.SparseMatrixCSC(ctx, A2)
    M1, M2 = api.JacobiPreconditioner(ctx, A1.diagonal()), api.JacobiPreconditioner(ctx, A2.diagonal())
    want1, want2 = api.pcg(fresh1, b1, x0, M1), api.pcg(fresh2, b2, x0, M2)
    assert before[1] > 3 and want1[1] > 3 and not np.array_equal(before[0], want1[0])

    def same_solve(got, want):
        return got[1] == want[1] and cases.same_bits(got[2], want[2]) and cases.same_bits(got[0], want[0])
    # numpy values
    vals1, rhs1 = dev.run(a1)
    A_op.set_values(vals1)
    assert cases.same_bits(A_op * x, fresh1 * x)
    M.refresh(A_op)
    assert cases.same_bits(M * x, M1 * x)
    assert same_solve(api.pcg(A_op, rhs1, x0, M), want1)               # replayed graphs see the new values
    # torch values, straight from a device run
    vt, bt = dev.run(torch.from_numpy(a2).cuda())
    A_op.set_values(vt)
    M.refresh(A_op)
    ctx.synchronize()
    assert cases.same_bits(A_op * x, fresh2 * x) and cases.same_bits(M * x, M2 * x)
    assert same_solve(api.pcg(A_op, bt.cpu().numpy(), x0, M), want2)
    # a scipy matrix
    A_op.set_values(A1)
    assert cases.same_bits(A_op * x, fresh1 * x)
    # update = run + set_values, for numpy and for torch coefficients
    bu = dev.update(a2, A_op)
    assert cases.same_bits(bu, b2) and cases.same_bits(A_op * x, fresh2 * x)
    but = dev.update(torch.from_numpy(a1).cuda(), A_op)
    M.refresh(A_op)
    ctx.synchronize()
    assert but.is_cuda and cases.same_bits(but.cpu().numpy(), b1) and cases.same_bits(A_op * x, fresh1 * x)
    assert same_solve(api.pcg(A_op, b1, x0, M), want1)
    for op in (A_op, fresh1, fresh2, M, M1, M2):
        op.close()
    dev.close()


def test_example06_loop_on_device_tensors(pkg, ctx, fem, grid60):
    """ξ -> KLField.coefficient -> FullAssemblyPlan.run -> A_op.set_values + AMGPreconditioner.set_values -> pcg, nothing on the
    host, against the same loop with the host assembly and a fresh SparseMatrixCSC per realization."""
    import torch
    api = pkg.api
    mesh, plan, _, ((A0, _), _, _) = grid60
    n = plan.n
    kl = fem.synthetic_kl(mesh.points)
    field = api.KLField(ctx, kl.Λ, kl.Ψ)
    dev = api.FullAssemblyPlan(ctx, plan)
    A_op = api.SparseMatrixCSC(ctx, A0)
    Π_dev, Π_host = api.AMGPreconditioner(ctx, A0, device_setup=True), api.AMGPreconditioner(ctx, A0, device_setup=True)
    rng = np.random.default_rng(481456)
    rhs = []
    for _ in range(2):
        ξ = torch.from_numpy(rng.standard_normal(kl.Λ.size)).cuda()
        a = field.coefficient(ξ)
        values, b = dev.run(a)
        A_op.set_values(values)
        Π_dev.set_values(values)
        x, it, res = api.pcg(A_op, b, torch.zeros(n, dtype=torch.float64, device="cuda"), Π_dev)
        ctx.synchronize()
        assert values.is_cuda and b.is_cuda and x.is_cuda
        # the host-assembled flow on the same coefficient
        a_h = a.cpu().numpy()
        _, A, b_h = cases.host_system(fem, mesh, a_h, f_m1, u0734)
        fresh = api.SparseMatrixCSC(ctx, A)
        Π_host.set_values(A)
        xh, ith, resh = api.pcg(fresh, torch.from_numpy(b_h).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda"), Π_host)
        ctx.synchronize()
        assert cases.same_bits(b.cpu().numpy(), b_h)
        assert it == ith and it > 2 and cases.same_bits(res, resh) and cases.same_bits(x.cpu().numpy(), xh.cpu().numpy())
        assert np.linalg.norm(b_h - A @ x.cpu().numpy()) <= 1e-5 * np.linalg.norm(b_h)
        rhs.append(b_h)
        fresh.close()
    assert not np.array_equal(rhs[0], rhs[1])            # f = -1 with a Dirichlet lift: b depends on the coefficient
    for op in (A_op, Π_dev, Π_host):
        op.close()
    dev.close()


def test_refusals_leave_operator_and_plan_usable(pkg, ctx, fem, grid60):
    import torch
    api = pkg.api
    Lb = ctx._L
    mesh, plan, (a0, a1, _), ((A0, b0), (A1, b1), _) = grid60
    n = plan.n
    dev = api.FullAssemblyPlan(ctx, plan)
    A_op = api.SparseMatrixCSC(ctx, A0)
    M = api.JacobiPreconditioner(ctx, A0.diagonal())
    x = np.random.default_rng(1).standard_normal(n)
    y0 = A_op * x
    # set_values on an operator that is not a CSR operator; a wrong-length array
    ctx._mode_for(x)
    with pytest.raises(api.MiError, match="mi_csr_set_values"):
        api.check(Lb.mi_csr_set_values(M._h, C.c_void_p(A0.data.ctypes.data)))
    with pytest.raises(api.MiError, match="mi_csr_set_values"):
        A_op.set_values(A0.data[:-1])
    with pytest.raises(api.MiError, match="mi_csr_set_values"):
        A_op.set_values(torch.zeros(plan.nnz + 1, dtype=torch.float64, device="cuda"))
    # a full plan in mi_assembly_run and a block plan in mi_full_assembly_run / _update
    generic = api.AssemblyPlan(ctx, plan.as_block_plan())
    out = np.empty(plan.n_entries)
    BAD = pkg._lib.MI_ERR_BAD_ARG
    vp = C.c_void_p
    assert Lb.mi_assembly_run(dev._h, vp(a0.ctypes.data), vp(out.ctypes.data)) == BAD and b"mi_full_assembly_run" in Lb.mi_last_error()
    assert Lb.mi_full_assembly_run(generic._h, vp(a0.ctypes.data), vp(out.ctypes.data), vp(out.ctypes.data)) == BAD
    assert Lb.mi_full_assembly_update(generic._h, vp(a0.ctypes.data), A_op._h, vp(out.ctypes.data)) == BAD
    with pytest.raises(api.MiError):
        api.AssemblyPlan.run(dev, a0)
    # update into an operator of another pattern or of another kind; refresh with a size mismatch or from no matrix
    small = api.SparseMatrixCSC(ctx, A0[:n - 1, :n - 1])
    with pytest.raises(api.MiError):
        dev.update(a1, small)
    idx = A0.indices.copy()
    idx[A0.indptr[1] - 1] += 1                                          # same rows, same count, one column moved
    moved = api.SparseMatrixCSC(ctx, (A0.indptr, idx, A0.data, n))
    with pytest.raises(api.MiError, match="pattern"):
        dev.update(a1, moved)
    with pytest.raises(api.MiError):
        dev.update(a1, M)
    with pytest.raises(api.MiError):
        api.JacobiPreconditioner(ctx, np.ones(n - 1)).refresh(A_op)
    with pytest.raises(api.MiError):
        M.refresh(M)
    with pytest.raises(api.MiError):
        api.JacobiOperator.refresh(api.IdentityPreconditioner(ctx, n), A_op)
    # a plan the mesh does not produce
    import copy
    bad = copy.copy(plan)
    bad.colidx = plan.colidx.copy(); bad.colidx[5] += 1
    with pytest.raises(api.MiError, match="colidx"):
        api.FullAssemblyPlan(ctx, bad)
    # everything still works
    assert cases.same_bits(A_op * x, y0) and cases.same_bits(M * x, (1.0 / A0.diagonal()) * x)
    vals, rhs = dev.run(a1)
    assert cases.same_bits(vals, A1.data) and cases.same_bits(rhs, b1)
    assert cases.same_bits(dev.update(a1, A_op), b1) and cases.same_bits(A_op * x, api.SparseMatrixCSC(ctx, A1) * x)
    assert cases.same_bits(generic.run(a1)[:plan.nnz], A1.data)
