"""Meshes, coefficients and the bitwise comparison shared by tests/test_full_assembly_cpu.py and tests/test_gpu_full_assembly.py.

  grid<N>   fem.get_mesh(N), N in {3, 4, 17, 18, 19}: 1, 4, 225, 256 and 289 free rows — one row with every neighbour Dirichlet,
            then one short of, exactly, and one past a row block of FA_ROWS = 256 rows
  unstructured   conftest.unstructured_mesh: permuted node and element numbers, rotated vertex order, jittered nodes
  fan<k>    a centre, a free ring of k nodes around it and a Dirichlet ring around that: the centre row stores k + 1 entries.
            k = 40: a row far longer than a grid's 7; k = FA_SEG - 1: the centre row exactly fills a row block. The centre is
            numbered in the middle of the free ring, so that row blocks end in front of it and start behind it.
"""
import numpy as np

GRID_SIZES = (3, 4, 17, 18, 19)


def f_var(x, y):
    return 1.0 + x - 2.0 * y * y


def f_zero(x, y):
    return 0.0 * x


def u_var(x, y):
    return x * x - y + 0.3


def fan_mesh(fem, k):
    """(Mesh without a neighbour table) of the fan with k spokes; nodes: ring 1 [0, h), the centre, ring 1 [h, k), ring 2."""
    h = k // 2
    θ = 2 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(θ), np.sin(θ)])
    points = np.concatenate([0.5 * ring[:, :h], np.zeros((2, 1)), 0.5 * ring[:, h:], ring], axis=1) * 0.5 + 0.5
    r1 = np.where(np.arange(k) < h, np.arange(k), np.arange(k) + 1)
    r2 = k + 1 + np.arange(k)
    nxt = (np.arange(k) + 1) % k
    centre = np.full(k, h)
    cells = np.concatenate([np.stack([centre, r1, r1[nxt]]), np.stack([r1, r2, r2[nxt]]), np.stack([r1, r2[nxt], r1[nxt]])], axis=1)
    # rotate the vertex order of every third element and interleave the three families: ascending element order then mixes them
    rot = np.arange(cells.shape[1]) % 3
    cells = np.take_along_axis(cells, (np.arange(3)[:, None] + rot[None, :]) % 3, 0)
    perm = np.random.default_rng(k).permutation(cells.shape[1])
    marker = np.zeros(2 * k + 1, dtype=np.int64)
    marker[r2] = 1
    return fem.Mesh(np.ascontiguousarray(cells[:, perm]).astype(np.int64), points, marker, None, 0)


def mesh_cases(fem, fans=(40,), grids=GRID_SIZES):
    """name -> Mesh"""
    from conftest import unstructured_mesh
    out = {f"grid{N}": fem.get_mesh(N) for N in grids}
    out["unstructured"] = unstructured_mesh(fem)[0]
    for k in fans:
        out[f"fan{k}"] = fan_mesh(fem, k)
    return out


def coefficients(fem, mesh):
    """a constant and a lognormal nodal coefficient"""
    from conftest import lognormal_coeff
    return {"constant": np.full(mesh.points.shape[1], 0.7), "lognormal": lognormal_coeff(fem, mesh.points, 5)}


def runs(fem, mesh):
    """(label, a, f, uexact): both coefficients with a non-constant f and uexact, and once f ≡ 0"""
    co = coefficients(fem, mesh)
    return [("constant", co["constant"], f_var, u_var), ("lognormal", co["lognormal"], f_var, u_var), ("lognormal, f = 0", co["lognormal"], f_zero, u_var)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def host_system(fem, mesh, a, f, uexact):
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    A, b = fem.do_isotropic_elliptic_assembly(mesh.cells, mesh.points, dinds, mesh.point_marker, a, f, uexact)
    return dinds, A, b


def make_plan(fem, mesh, f, uexact):
    dinds = fem.get_dirichlet_inds(mesh.points, mesh.point_marker)
    return fem.make_full_assembly_plan(mesh.cells, mesh.points, dinds, mesh.point_marker, f, uexact)
