"""Host checks (no GPU) of the row-owned full-system assembly plan. All comparisons are BITWISE (values and their sign bits):
the same operations in the same order leave no room for a tolerance.

  * fem.FullAssemblyPlan.run(a) equals fem.do_isotropic_elliptic_assembly (pattern, values, b); so does
    oracle.run_assembly_plan on plan.as_block_plan(); plan.system round-trips — on every mesh of full_assembly_cases, the fan
    whose centre row exactly fills a row block included, with a constant and a lognormal coefficient and once with f ≡ 0;
  * the row blocks: at most FA_ROWS rows, at most FA_SEG stored entries, no split row, greedy;
  * csrc/full_assembly_plan.hpp through tests/cpp/full_assembly_plan_check.cpp, plain and under -fsanitize=address,undefined:
    the arrays of the python mirror, 0- and 1-based; every refusal by name, the fan with k = FA_SEG among them;
  * the ABI: prototypes present, NULL handles refused without a device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import full_assembly_cases as cases
from conftest import ROOT

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
PLAN_ARRAYS = ("node_row", "rowptr", "colidx", "diag_pos", "inc_ptr", "inc_code", "inc_pos", "blk_row")


@pytest.fixture(scope="module")
def meshes(fem):
    return cases.mesh_cases(fem, fans=(40, fem.FA_SEG - 1))


# --------------------------------------------------------------------------------------------------- the numbers
def test_row_owned_run_has_the_bits_of_the_host_assembly(fem, orc, meshes):
    for name, mesh in meshes.items():
        for label, a, f, uexact in cases.runs(fem, mesh):
            dinds, A, b = cases.host_system(fem, mesh, a, f, uexact)
            plan = cases.make_plan(fem, mesh, f, uexact)
            assert np.array_equal(plan.rowptr, A.indptr) and np.array_equal(plan.colidx, A.indices), (name, label)
            vals, rhs = plan.run(a)
            assert cases.same_bits(vals, A.data) and cases.same_bits(rhs, b), (name, label)
            out = orc.run_assembly_plan(plan.as_block_plan(), a)
            assert out.size == plan.n_entries == plan.nnz + plan.n
            assert cases.same_bits(out[:plan.nnz], A.data) and cases.same_bits(out[plan.nnz:], b), (name, label)
            A2, b2 = plan.system(vals, rhs)
            assert (A2 != A).nnz == 0 and cases.same_bits(A2.data, A.data) and np.array_equal(A2.indices, A.indices)
            assert np.array_equal(A2.indptr, A.indptr) and cases.same_bits(b2, b) and A2.shape == A.shape
            assert cases.same_bits(A2.T.tocsr().data, A.data)              # bitwise symmetric: CSR and CSC coincide


def test_the_cases_hold_what_they_promise(fem, meshes):
    rows = {name: cases.make_plan(fem, m, cases.f_var, cases.u_var) for name, m in meshes.items()}
    assert [rows[f"grid{N}"].n for N in cases.GRID_SIZES] == [1, 4, 225, 256, 289]
    p = rows["grid3"]
    assert p.nnz == 1 and np.all((p.inc_pos & 0xFFFF) == fem.FA_DIR) and np.all(p.inc_pos >> 16 == fem.FA_DIR)   # every neighbour is Dirichlet
    assert [rows[f"grid{N}"].blk_row.size - 1 for N in (17, 18, 19)] == [1, 1, 2]
    # structured meshes store exact zeros, one per hypotenuse: 450 of the 1 666 entries at N = 18
    p = rows["grid18"]
    vals, _ = p.run(np.ones(p.n_node))
    assert p.nnz == 1666 and int((vals == 0).sum()) == 450
    assert np.diff(rows["fan40"].rowptr).max() == 41
    p = rows[f"fan{fem.FA_SEG - 1}"]
    centre = int(np.argmax(np.diff(p.rowptr)))
    assert np.diff(p.rowptr)[centre] == fem.FA_SEG and centre in p.blk_row and centre + 1 in p.blk_row   # a block of its own
    assert 0 < centre < p.n - 1
    for p in rows.values():
        r, s = np.diff(p.blk_row), np.diff(p.rowptr[p.blk_row])
        assert p.blk_row[0] == 0 and p.blk_row[-1] == p.n and np.all(r >= 1) and np.all(r <= fem.FA_ROWS) and np.all(s <= fem.FA_SEG)
        for k in range(1, p.blk_row.size - 1):       # greedy: the next row would not have fitted
            r0, r1 = p.blk_row[k - 1], p.blk_row[k]
            assert r1 - r0 == fem.FA_ROWS or p.rowptr[r1 + 1] - p.rowptr[r0] > fem.FA_SEG
        assert np.array_equal(p.colidx[p.rowptr[:-1] + p.diag_pos], np.arange(p.n))


def test_python_refusals_name_the_offender(fem):
    m = fem.get_mesh(5)
    d = fem.get_dirichlet_inds(m.points, m.point_marker)

    def plan(cells=m.cells, points=m.points):
        return fem.make_full_assembly_plan(cells, points, d, m.point_marker, cases.f_var, cases.u_var)
    c = m.cells.copy(); c[1, 7] = 25
    with pytest.raises(ValueError, match="element 7, vertex 1: node 25 is outside"):
        plan(cells=c)
    c = m.cells.copy(); c[2, 3] = c[0, 3]
    with pytest.raises(ValueError, match=f"element 3 lists node {c[0, 3]} twice"):
        plan(cells=c)
    p = m.points.copy(); p[:, m.cells[1, 9]] = p[:, m.cells[0, 9]]
    with pytest.raises(ValueError, match="element [0-9]+ has zero area"):
        plan(points=p)
    k = fem.FA_SEG
    fan = cases.fan_mesh(fem, k)
    with pytest.raises(ValueError, match=f"row {k // 2} has {k + 1} stored entries, more than FA_SEG = {k}"):
        cases.make_plan(fem, fan, cases.f_var, cases.u_var)


# --------------------------------------------------------------------------------------------------- the plan checker
def _build(tmp, flags=()):
    exe = str(tmp / ("full_assembly_plan_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "full_assembly_plan_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fa_plan"))


@pytest.fixture(scope="module")
def sanitized_checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fa_plan_san"), SANITIZE)


def _arr(a, shift=0):
    a = np.asarray(a, dtype=np.int64).ravel()
    return " ".join(str(v) for v in [a.size, *(a + shift)])


def write_case(path, cells, points, marker, rowptr=None, colidx=None, base=0, nel=None, n=None):
    cells, points, marker = np.asarray(cells), np.asarray(points, dtype=np.float64), np.asarray(marker)
    with_pattern = rowptr is not None
    rowptr = np.zeros(0, dtype=np.int64) if rowptr is None else np.asarray(rowptr)
    colidx = np.zeros(0, dtype=np.int64) if colidx is None else np.asarray(colidx)
    head = f"{cells.shape[1] if nel is None else nel} {points.shape[1]} {base} {(rowptr.size - 1 if with_pattern else -1) if n is None else n} {int(with_pattern)}"
    pts = " ".join([str(points.size), *(float(v).hex() for v in points.ravel())])
    path.write_text("\n".join([head, _arr(cells, base), _arr(marker), _arr(rowptr, base), _arr(colidx, base), pts]) + "\n")
    return path


def run(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.splitlines()[0])


def test_plan_arrays_equal_the_python_mirror(fem, meshes, checker, sanitized_checker, tmp_path):
    for name, mesh in meshes.items():
        plan = cases.make_plan(fem, mesh, cases.f_var, cases.u_var)
        for base in (0, 1):
            for with_pattern in (False, True):
                pat = (plan.rowptr, plan.colidx) if with_pattern else (None, None)
                p = write_case(tmp_path / f"{name}_{base}_{int(with_pattern)}.txt", mesh.cells, mesh.points, mesh.point_marker, *pat, base=base)
                doc = run(checker, p)
                assert doc["status"] == 0 and doc["err"] == "", (name, doc["err"])
                assert (doc["fa_rows"], doc["fa_seg"], doc["fa_dir"]) == (fem.FA_ROWS, fem.FA_SEG, fem.FA_DIR)
                assert doc["n"] == plan.n and doc["bytes"] == plan.bytes()
                assert doc["cells"] == list(mesh.cells.ravel())
                for key in PLAN_ARRAYS:
                    assert doc[key] == list(getattr(plan, key)), (name, base, key)
                assert run(sanitized_checker, p) == doc


def test_plan_refusals_name_the_offender(fem, checker, sanitized_checker, tmp_path):
    m = fem.get_mesh(5)
    good = cases.make_plan(fem, m, cases.f_var, cases.u_var)
    kw = dict(cells=m.cells, points=m.points, marker=m.point_marker)
    outside, negative, twice, flat = m.cells.copy(), m.cells.copy(), m.cells.copy(), m.points.copy()
    outside[1, 7] = 25
    negative[0, 2] = -1
    twice[2, 3] = twice[0, 3]
    flat[:, m.cells[1, 9]] = flat[:, m.cells[0, 9]]
    flat_first = int(np.flatnonzero((m.cells == m.cells[1, 9]).any(axis=0) & (m.cells == m.cells[0, 9]).any(axis=0))[0])
    rp_bad, ci_bad = good.rowptr.copy(), good.colidx.copy()
    rp_bad[4] += 1
    ci_bad[11] += 1
    k = fem.FA_SEG
    fan = cases.fan_mesh(fem, k)
    bad = {
        "element 7, vertex 1: node 25 is outside": dict(kw, cells=outside),
        "element 2, vertex 0: node -1 is outside": dict(kw, cells=negative),
        f"element 3 lists node {twice[0, 3]} twice": dict(kw, cells=twice),
        f"element {flat_first} has zero area": dict(kw, points=flat),
        f"row {k // 2} has {k + 1} stored entries, more than FA_SEG = {k}": dict(cells=fan.cells, points=fan.points, marker=fan.point_marker),
        f"nel = {2 ** 29} elements: 4 nel = {2 ** 31} does not fit 31 bits": dict(kw, nel=2 ** 29),
        "nel = 0 elements": dict(kw, nel=0),
        "index_base = 2": dict(kw, base=2),
        f"the pattern has n = {good.n + 1} rows, the mesh has {good.n} free nodes": dict(kw, rowptr=np.append(good.rowptr, good.nnz), colidx=good.colidx),
        f"rowptr[4] = {rp_bad[4]}, the mesh gives {good.rowptr[4]}": dict(kw, rowptr=rp_bad, colidx=good.colidx),
        f"colidx[11] = {ci_bad[11]}, the mesh gives {good.colidx[11]}": dict(kw, rowptr=good.rowptr, colidx=ci_bad),
    }
    for j, (needle, case) in enumerate(bad.items()):
        p = write_case(tmp_path / f"bad{j}.txt", **case)
        for exe in (checker, sanitized_checker):
            doc = run(exe, p)
            assert doc["status"] == 1 and needle in doc["err"] and len(doc["err"]) > 40 and "rowptr" not in doc, (needle, doc)


# --------------------------------------------------------------------------------------------------- ABI
def test_prototypes_and_hostside_refusals(pkg):
    Lb = pkg._lib.load()
    hdr = open(os.path.join(ROOT, "include", "mi355schur.h")).read()
    for nm in ("mi_full_assembly_plan_create", "mi_full_assembly_run", "mi_full_assembly_update", "mi_full_assembly_stats",
               "mi_csr_set_values", "mi_diag_set_from_csr"):
        assert nm in pkg._lib.SIGNATURES and hasattr(Lb, nm) and f"int {nm}(" in hdr
    assert Lb.mi_version() >= 400
    BAD = pkg._lib.MI_ERR_BAD_ARG
    h = C.c_void_p(77)
    i64 = C.c_int64
    assert Lb.mi_full_assembly_plan_create(None, i64(1), i64(3), None, 0, None, None, i64(1), None, None, None, None, C.byref(h)) == BAD and not h.value
    assert Lb.mi_full_assembly_run(None, None, None, None) == BAD and Lb.mi_full_assembly_update(None, None, None, None) == BAD
    assert Lb.mi_csr_set_values(None, None) == BAD and Lb.mi_diag_set_from_csr(None, None) == BAD
    assert Lb.mi_full_assembly_stats(None, None, None, None) == BAD
