"""Host checks (no GPU) of the realization sampler:

  * the restatements of tests/kl_field_ref.py agree with fem.set_field / fem.draw (bits), fem.draw_dd_field and
    fem.get_kl_coordinates (rounding);
  * the dense and the factored form agree: fem.project_on_mesh then set_field, against the factored loop, within the
    factored bound (kl_field_ref.dd_bound);
  * the samplers of api.py (field=None: everything on the host) reproduce the restated chains under a scripted generator whose
    script holds a first-proposal acceptance, a run of two rejections and the ‖χ‖² <= ‖ξ‖² branch; cnt totals match; the hybrid
    sampler redraws its tail;
  * the ABI: prototypes present, mi_kl_field_tiling total and monotone on edge sizes, refusals without a device;
  * csrc/kl_field_plan.hpp through tests/cpp/kl_field_plan_check.cpp: offsets, tiles and owner lists against numpy, every
    refusal with a message that names the offender; the same checker under -fsanitize=address,undefined."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import kl_field_ref as ref
from conftest import ROOT

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


# --------------------------------------------------------------------------------------------------- restatements
def test_set_field_restatement_has_the_bits_of_fem(fem):
    rng = np.random.default_rng(0)
    Λ, Ψ = ref.small_modes(rng, 211, 9)
    Λ[4] = 0.0
    ξ = rng.standard_normal(9)
    g = fem.set_field(Λ, Ψ, ξ)
    assert np.array_equal(g, ref.set_field(Λ, Ψ, ξ))
    ξd, gd = fem.draw(fem.SyntheticKL(Λ, Ψ), np.random.default_rng(3))
    assert np.array_equal(gd, fem.set_field(Λ, Ψ, ξd)) and np.array_equal(gd, ref.set_field(Λ, Ψ, ξd))
    bad = ξ.copy(); bad[2] = np.nan
    assert np.all(np.isnan(fem.set_field(Λ, Ψ, bad)[Ψ[:, 2] != 0]))


def test_factored_restatement_agrees_with_fem_and_with_the_dense_form(fem):
    mesh, l2gd, elemsd, Φd, Φ, Λ, rng = ref.split_problem(fem)
    n = mesh.points.shape[1]
    cnt = np.bincount(np.concatenate(l2gd), minlength=n)
    assert set(cnt) == {1, 2, 4}
    ξ = rng.standard_normal(Λ.size)
    want = ref.dd_field(n, Λ, Φ, Φd, l2gd, ξ)
    bound = ref.dd_bound(n, Λ, Φ, Φd, l2gd, ξ)
    got = fem.draw_dd_field(n, Λ, Φ, Φd, l2gd, ξ)
    assert np.all(bound > 0) and np.all(np.abs(got - want) <= bound)
    Ψ = fem.project_on_mesh(n, Φ, elemsd, l2gd, Φd)
    dense = fem.set_field(Λ, Ψ, ξ)
    err = np.abs(dense - want)
    print(f"dense vs factored: max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)       # the dense side: md + cnt + 1 roundings in the projection, m + 3 in set_field — one side's budget
    assert np.abs(want).max() > 1e6 * bound.max()           # the bound is a rounding bound, not a loose one


def test_coordinates_restatement_and_round_trip(fem):
    import scipy.linalg as sla
    mesh = fem.get_mesh(7)
    M = fem.get_mass_matrix(mesh.cells, mesh.points)
    n, m = M.shape[0], 6
    rng = np.random.default_rng(2)
    X = rng.standard_normal((n, m))
    Ψ = X @ np.linalg.inv(sla.cholesky(X.T @ (M @ X)))      # Ψ' M Ψ = I
    Λ = np.sort(rng.random(m) + 0.1)[::-1]
    ξ = rng.standard_normal(m)
    g = fem.set_field(Λ, Ψ, ξ)
    got, want = fem.get_kl_coordinates(g, Λ, Ψ, M), ref.kl_coordinates(g, Λ, Ψ, M)
    assert np.all(np.abs(got - want) <= ref.coords_bound(g, Λ, Ψ, M))
    assert np.abs(got - ξ).max() <= 1e-12 * max(1.0, np.abs(ξ).max())


# --------------------------------------------------------------------------------------------------- samplers
def test_mcmc_chain_matches_the_restatement_under_the_script(pkg):
    rng = np.random.default_rng(4)
    Λ, Ψ = ref.small_modes(rng, 37, 3)
    want, trace = ref.mcmc_chain(Λ, Ψ, ref.ScriptedRng(ref.mcmc_script()), 3)
    # the script holds what it promises
    assert len(trace[0]) == 1 and trace[0][0][0] and trace[0][0][1] < 1.0 and trace[0][0][2] <= trace[0][0][1]
    assert len(trace[1]) == 3 and all(u > α for _, α, u in trace[1][:2]) and trace[1][2][2] <= trace[1][2][1]
    assert len(trace[2]) == 1 and not trace[2][0][0] and trace[2][0][1] == 1.0
    script = ref.ScriptedRng(ref.mcmc_script())
    s = pkg.api.McmcSampler(Λ, Ψ, script)
    assert s.σ2 == 1.0 and s.ϑ2 == 2.38 ** 2 * 1.0 / 3 and s.χ.shape == (3,)
    assert np.array_equal(s.ξ, want[0][0]) and np.array_equal(s.g, want[0][1]) and np.array_equal(s.a, np.exp(s.g))
    cnts = []
    for ξ, g, cnt in want[1:]:
        cnts.append(s.draw())
        assert cnts[-1] == cnt and np.array_equal(s.ξ, ξ) and np.array_equal(s.g, g) and np.array_equal(s.χ, s.ξ)
    assert cnts == [1, 3, 1] and sum(cnts) == sum(w[2] for w in want) and script.exhausted()
    s.set([1.0, 2.0, 3.0])
    assert np.array_equal(s.g, ref.set_field(Λ, Ψ, [1.0, 2.0, 3.0])) and np.array_equal(s.ξ, [1.0, 2.0, 3.0])


def test_mc_and_hybrid_samplers(pkg):
    rng = np.random.default_rng(5)
    Λ, Ψ = ref.small_modes(rng, 23, 4)
    normals = [("normal", list(rng.standard_normal(4))) for _ in range(3)]
    want = ref.mc_chain(Λ, Ψ, ref.ScriptedRng(normals), 2)
    s = pkg.api.McSampler(Λ, Ψ, ref.ScriptedRng(normals))
    for k, (ξ, g) in enumerate(want):
        if k:
            assert s.draw() is None
        assert np.array_equal(s.ξ, ξ) and np.array_equal(s.g, g) and np.array_equal(s.a, np.exp(g))
    # hybrid: Metropolis on the first two coordinates, a fresh tail per draw
    want = ref.hybrid_chain(Λ, Ψ, 2, ref.ScriptedRng(ref.hybrid_script()), 2)
    script = ref.ScriptedRng(ref.hybrid_script())
    h = pkg.api.HybridSampler(Λ, Ψ, script, 2)
    assert h.ϑ2 == 2.38 ** 2 / 2 and np.array_equal(h.ξ, want[0][0]) and np.array_equal(h.g, want[0][1])
    for (ξ, g, cnt), tail in zip(want[1:], ([-0.9, 0.6], [1.3, 0.4])):
        assert h.draw() == cnt
        assert np.array_equal(h.ξ, ξ) and np.array_equal(h.g, g) and np.array_equal(h.ξ[2:], tail)
    assert [w[2] for w in want] == [0, 1, 2] and script.exhausted()
    with pytest.raises(ValueError):
        pkg.api.HybridSampler(Λ, Ψ, ref.ScriptedRng([]), 5)
    # a real generator: the documented call order reproduces the chain
    a, b = pkg.api.McmcSampler(Λ, Ψ, np.random.default_rng(9)), np.random.default_rng(9)
    ξ0 = b.standard_normal(4); b.standard_normal(4)
    assert np.array_equal(a.ξ, ξ0)
    total = sum(a.draw() for _ in range(20))
    assert total >= 20 and np.all(np.isfinite(a.g))


# --------------------------------------------------------------------------------------------------- ABI
def test_prototypes_tiling_and_hostside_refusals(pkg):
    Lb = pkg._lib.load()
    names = ["mi_kl_field_create", "mi_kl_field_create_dd", "mi_kl_field_set", "mi_kl_field_coords", "mi_kl_field_tiling",
             "mi_kl_field_stats", "mi_kl_field_destroy"]
    hdr = open(os.path.join(ROOT, "include", "mi355schur.h")).read()
    for nm in names:
        assert nm in pkg._lib.SIGNATURES and hasattr(Lb, nm) and f"int {nm}(" in hdr
    assert "typedef struct mi_kl_field_s *mi_kl_field_t;" in hdr
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1, 1)
    assert rt >= 64 and rt % 64 == 0 and mc >= 1 and rb == 8
    # total on the edge sizes, constant tile sizes, splits monotone in n and never more than the row tiles
    last = 0
    for n in (1, rt - 1, rt, rt + 1, 2 * rt, 2 * rt + 1, 17 * rt + 5, 1000 * rt, 2 ** 30):
        for m in (1, 2, mc - 1, mc, mc + 1, 1000):
            for nreal in (1, rb - 1, rb, rb + 1, 2 * rb + 1):
                t = pkg.api.kl_field_tiling(n, m, nreal)
                assert t[:3] == (rt, mc, rb) and 1 <= t[3] <= (n + rt - 1) // rt
                assert t[3] == pkg.api.kl_field_tiling(n, m, 1)[3]
        s = pkg.api.kl_field_tiling(n, 64, 1)[3]
        assert s >= last
        last = s
    assert pkg.api.kl_field_tiling(rt, 1)[3] == 1 and pkg.api.kl_field_tiling(rt + 1, 1)[3] == 2
    BAD = pkg._lib.MI_ERR_BAD_ARG
    i64 = C.c_int64
    for n, m, nreal in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 1, 1), (2 ** 30 + 1, 1, 1)):
        assert Lb.mi_kl_field_tiling(i64(n), i64(m), i64(nreal), None, None, None, None) == BAD
        assert Lb.mi_last_error().decode().startswith("mi_kl_field_tiling")
    assert Lb.mi_kl_field_tiling(i64(5), i64(5), i64(5), None, None, None, None) == 0
    # NULL handles are refused before any device work; destroying NULL is a no-op
    assert Lb.mi_kl_field_set(None, i64(1), None, i64(1), None, i64(1), None, i64(1)) == BAD
    assert Lb.mi_kl_field_coords(None, None, None, None) == BAD and Lb.mi_kl_field_stats(None, None, None) == BAD
    h = C.c_void_p(77)
    assert Lb.mi_kl_field_create(None, i64(3), i64(1), None, None, i64(3), C.byref(h)) == BAD and not h.value
    assert Lb.mi_kl_field_destroy(None) == 0


# --------------------------------------------------------------------------------------------------- the plan checker
def _build(tmp, flags=()):
    exe = str(tmp / ("kl_field_plan_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "kl_field_plan_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("klf_plan"))


@pytest.fixture(scope="module")
def sanitized_checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("klf_plan_san"), SANITIZE)


def _arr(a, shift=0):
    a = np.asarray(a, dtype=np.int64).ravel()
    return " ".join(str(v) for v in [a.size, *(a + shift)])


def write_plan(path, n, maps, md, base=0, n_d=None, ndom=None):
    n_d = [len(l) for l in maps] if n_d is None else n_d
    inds = np.concatenate([np.asarray(l, dtype=np.int64) for l in maps]) if maps else np.zeros(0, dtype=np.int64)
    path.write_text("\n".join([f"plan {n} {len(maps) if ndom is None else ndom} {base}", _arr(n_d), _arr(md), _arr(inds, base)]) + "\n")
    return path


def run(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.splitlines()[0])


def check_plan(doc, n, maps, md, rt):
    assert doc["status"] == 0 and doc["err"] == ""
    n_d = np.array([len(l) for l in maps])
    assert doc["nloc"] == n_d.sum() and doc["nred"] == sum(md) and doc["md_max"] == max(md)
    assert doc["y_off"] == [0, *np.cumsum(md)] and doc["t_off"] == [0, *np.cumsum(n_d)] and doc["phid_off"] == [0, *np.cumsum(n_d * np.array(md))]
    tiles = [(d, r0) for d in range(len(maps)) for r0 in range(0, len(maps[d]), rt)]
    assert list(zip(doc["tile_d"], doc["tile_row0"])) == tiles
    flat = np.concatenate(maps)
    cnt = np.bincount(flat, minlength=n)
    assert doc["cnt_max"] == cnt.max() and doc["own_ptr"] == [0, *np.cumsum(cnt)]
    order = np.lexsort((np.arange(flat.size), flat))          # by node, then by position: ascending subdomain
    assert doc["own_pos"] == list(order)
    assert doc["bytes"] == 4 * (4 * len(maps) + 2 + 2 * len(tiles) + n + 1 + flat.size) + 8 * (len(maps) + 1)


def plan_cases(fem, rt):
    """(n, maps, md): the 2 x 2 split with a subdomain below a row tile and one that crosses a tile edge by one row; a single
    subdomain; many owners of one node"""
    mesh, l2gd, _, _, _, _, _ = ref.split_problem(fem)
    assert l2gd[0].size == rt + 1 and all(l.size < rt for l in l2gd[1:])
    rng = np.random.default_rng(6)
    n = rt + 1
    yield mesh.points.shape[1], l2gd, (1, 3, 7, 2)
    yield n, [rng.permutation(n)], (4,)
    yield n, [rng.permutation(n), np.arange(3), np.array([n - 1, 0]), rng.permutation(n)[:rt]], (2, 1, 70, 3)
    yield 1, [np.array([0])] * 5, (1, 1, 2, 1, 1)


def test_plan_against_numpy(fem, pkg, checker, sanitized_checker, tmp_path):
    rt = pkg.api.kl_field_tiling(1, 1)[0]
    for k, (n, maps, md) in enumerate(plan_cases(fem, rt)):
        for base in (0, 1):
            p = write_plan(tmp_path / f"case{k}_{base}.txt", n, maps, md, base)
            doc = run(checker, p)
            check_plan(doc, n, maps, md, rt)
            assert run(sanitized_checker, p) == doc


def test_tiling_through_the_header_equals_the_abi(pkg, checker, sanitized_checker, tmp_path):
    rt, mc, rb, _ = pkg.api.kl_field_tiling(1, 1)
    for k, (n, m, nreal) in enumerate([(1, 1, 1), (rt, mc, rb), (rt + 1, mc + 1, rb + 1), (10 ** 6, 64, 1), (2 ** 30, 2 ** 30, 2 ** 30), (5000, 1, 3)]):
        p = tmp_path / f"tiling{k}.txt"
        p.write_text(f"tiling {n} {m} {nreal}\n")
        doc = run(checker, p)
        assert run(sanitized_checker, p) == doc
        assert (doc["row_tile"], doc["mode_chunk"], doc["real_block"], doc["coord_splits"]) == pkg.api.kl_field_tiling(n, m, nreal)
        assert doc["row_tiles"] == -(-n // rt) and doc["real_blocks"] == -(-nreal // rb) and doc["coord_col_blocks"] == -(-m // rb)
        assert (doc["coord_splits"] - 1) * doc["coord_tiles_per_split"] < doc["row_tiles"] <= doc["coord_splits"] * doc["coord_tiles_per_split"]
        assert doc["rb_in_use"] in (1, 2, 4, rb) and doc["rb_in_use"] >= min(nreal, rb)


def test_plan_refusals_name_the_offender(checker, sanitized_checker, tmp_path):
    good = [np.array([0, 1, 2]), np.array([2, 3])]
    cases = {
        "n = 0": dict(n=0, maps=good, md=(1, 1)),
        "ndom = 0": dict(n=4, maps=[], md=()),
        "md[1] = 0": dict(n=4, maps=good, md=(2, 0)),
        "n_d[0] = 0": dict(n=4, maps=good, md=(1, 1), n_d=[0, 2]),
        "n_d[1] = 9": dict(n=4, maps=good, md=(1, 1), n_d=[3, 9]),
        "node 4 is outside": dict(n=4, maps=[np.array([0, 1, 4]), np.array([2, 3])], md=(1, 1)),
        "node -1 is outside": dict(n=4, maps=[np.array([0, -1, 1]), np.array([2, 3])], md=(1, 1)),
        "lists node 1 twice": dict(n=4, maps=[np.array([0, 1, 2, 1]), np.array([3])], md=(1, 1)),
        "node 3 belongs to no subdomain": dict(n=4, maps=[np.array([0, 1, 2]), np.array([2, 0])], md=(1, 1)),
        "index_base = 2": dict(n=4, maps=good, md=(1, 1), base=2),
    }
    for k, (needle, kw) in enumerate(cases.items()):
        p = write_plan(tmp_path / f"bad{k}.txt", **kw)
        for exe in (checker, sanitized_checker):
            doc = run(exe, p)
            assert doc["status"] == 1 and needle in doc["err"] and len(doc["err"]) > 40 and "own_ptr" not in doc, (needle, doc)
