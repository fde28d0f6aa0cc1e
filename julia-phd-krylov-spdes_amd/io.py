"""The reference's on-disk formats, so that meshes / partitions produced by the Julia
pipeline (Triangle + METIS) can be fed to this library and its outputs read by the reference's `*.py` plots.

NPZ.jl's `npzwrite(filename, array)` writes ONE array in NPY format whatever the file extension is, so the
reference's `data/*.npz` files are NPY files; numpy.load recognises them by their magic bytes.

  Fem/Mesh.jl:49-55   save_mesh:       cells' .- 1 (nel x 3, 0-based), points' (nnode x 2),
                                       point_markers' (nnode x 1), cell_neighbors' (nel x 3, as TriangleMesh gives them)
  Fem/Mesh.jl:84-91   load_mesh:       the inverse (cells .+ 1)
  Fem/Mesh.jl:216-219 save_partition:  epart .- 1, npart .- 1
  Example07:281-285   iteration counts as a 1-D integer array
  Example02:41-42, Example04:92-93   KL pairs: `data/<root>.kl-eigvals.npz` (nvec,), `.kl-eigvecs.npz` (nnode x nvec),
                                     <root> = get_root_filename(model, sig2, L, tentative_nnode)

In memory this package is 0-based with -1 as the boundary tag of `cell_neighbors` (fem.Mesh).
"""
from __future__ import annotations

import os

import numpy as np

from .fem import Mesh


def _write(path: str, a: np.ndarray) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:           # a file object: numpy must not append ".npy"
        np.save(fh, np.asfortranarray(a))  # Julia arrays are column-major; NPZ.jl sets fortran_order


def mesh_paths(data_dir: str, tentative_nnode: int):
    root = os.path.join(data_dir, f"DoF{tentative_nnode}")
    return {k: f"{root}.{k}.npz" for k in ("cells", "points", "point_markers", "cell_neighbors")}


def save_mesh(mesh: Mesh, tentative_nnode: int, data_dir: str = "data") -> None:
    """`save_mesh(mesh, tentative_nnode)` (Fem/Mesh.jl:49-55). Neighbours are written 1-based with -1 on the
    boundary, the convention `set_subdomains` expects after its TriangleMesh correction (EPDD.jl:106-111)."""
    p = mesh_paths(data_dir, tentative_nnode)
    _write(p["cells"], mesh.cells.T.astype(np.int64))
    _write(p["points"], mesh.points.T.astype(np.float64))
    _write(p["point_markers"], mesh.point_marker.reshape(-1, 1).astype(np.int64))
    nb = np.where(mesh.cell_neighbors < 0, -1, mesh.cell_neighbors + 1)
    _write(p["cell_neighbors"], nb.T.astype(np.int64))


def load_mesh(tentative_nnode: int, data_dir: str = "data") -> Mesh:
    """`load_mesh(tentative_nnode)` (Fem/Mesh.jl:84-91) + the neighbour-index correction of
    `set_subdomains` (EPDD.jl:106-111: if the largest neighbour index exceeds nel the table is shifted by one
    and the boundary tag is -1; otherwise the smallest entry is the boundary tag)."""
    p = mesh_paths(data_dir, tentative_nnode)
    cells = np.load(p["cells"]).astype(np.int64).T.copy()                 # (3, nel), already 0-based on disk
    points = np.load(p["points"]).astype(np.float64).T.copy()             # (2, nnode)
    marker = np.load(p["point_markers"]).astype(np.int64).ravel()
    nb = np.load(p["cell_neighbors"]).astype(np.int64).T.copy()           # (3, nel), Julia/Triangle numbering
    nel = cells.shape[1]
    bnd_tag, iel_max = int(nb.min()), int(nb.max())
    if iel_max > nel:
        nb = nb - 1
        bnd_tag = -1
    nb0 = np.where(nb == bnd_tag, -1, nb - 1)                             # 1-based -> 0-based, -1 = boundary
    n_side = int(round(np.sqrt(points.shape[1])))
    return Mesh(cells, points, marker, nb0, n_side)


def partition_paths(data_dir: str, tentative_nnode: int, ndom: int):
    root = os.path.join(data_dir, f"DoF{tentative_nnode}-ndom{ndom}")
    return f"{root}.epart.npz", f"{root}.npart.npz"


def save_partition(epart, npart, tentative_nnode: int, ndom: int, data_dir: str = "data") -> None:
    """`save_partition` (Fem/Mesh.jl:216-219): 0-based subdomain ids on disk."""
    pe, pn = partition_paths(data_dir, tentative_nnode, ndom)
    _write(pe, np.asarray(epart, dtype=np.int64))
    _write(pn, np.asarray(npart, dtype=np.int64))


def load_partition(tentative_nnode: int, ndom: int, data_dir: str = "data"):
    """`load_partition` (Fem/Mesh.jl:243-247); returned 0-based (the reference adds 1 for Julia)."""
    pe, pn = partition_paths(data_dir, tentative_nnode, ndom)
    return np.load(pe).astype(np.int64).ravel(), np.load(pn).astype(np.int64).ravel()


def save_pcg_iters(iters, root_fname: str, ndom: int, tag: str, nreals: int, data_dir: str = "data",
                   precond: str = "neumann-neumann") -> str:
    """Example07:284-285: `data/$root_fname.neumann-neumann_ndom$ndom_$tag.pcg-iters.nreals$nreals.npz`;
    `precond="A_GG"`: Example07:423-424, `data/$root_fname.A_GG_ndom$ndom_$tag.pcg-iters.nreals$nreals.npz`."""
    path = os.path.join(data_dir, f"{root_fname}.{precond}_ndom{ndom}_{tag}.pcg-iters.nreals{nreals}.npz")
    _write(path, np.asarray(iters, dtype=np.int64))
    return path


def _julia_float(v: float) -> str:
    """How Julia interpolates a Float64 into a string (`"$v"`): the shortest digits that round-trip, always with a decimal
    point (1.0, 0.1); exponent form (`1.0e-5`, `1.0e6`) below 1e-4 and from 1e6."""
    v = float(v)
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "Inf" if v > 0 else "-Inf"
    r = repr(v)
    if "e" in r:
        mant, exp = r.split("e")
        e = int(exp)
    elif abs(v) >= 1e6:
        sign = "-" if r.startswith("-") else ""
        whole, frac = r.lstrip("-").split(".")
        e = len(whole) - 1
        digits = (whole + frac).rstrip("0") or "0"
        mant = sign + digits[0] + "." + (digits[1:] or "0")
    else:
        return r
    if "." not in mant:
        mant += ".0"
    return f"{mant}e{e}"


def get_root_filename(model: str, sig2: float, L: float, nnode: int) -> str:
    """`get_root_filename(model, sig2, L, nnode)` (KarhunenLoeveDomainDecompositionHelper.jl:72-80):
    "SExp_sig21.0_L0.1_DoF4000"."""
    return f"{model}_sig2{_julia_float(sig2)}_L{_julia_float(L)}_DoF{int(nnode)}"


def kl_paths(root_fname: str, data_dir: str = "data"):
    root = os.path.join(data_dir, root_fname)
    return f"{root}.kl-eigvals.npz", f"{root}.kl-eigvecs.npz"


def save_kl(Λ, Ψ, root_fname: str, data_dir: str = "data"):
    """Example02:41-42 / Example04:92-93: `npzwrite("data/$root_fname.kl-eigvals.npz", Λ)` and `.kl-eigvecs.npz` (nnode x nvec)."""
    pv, pe = kl_paths(root_fname, data_dir)
    _write(pv, np.asarray(Λ, dtype=np.float64))
    _write(pe, np.asarray(Ψ, dtype=np.float64))
    return pv, pe


def load_kl(root_fname: str, data_dir: str = "data"):
    """The inverse of save_kl -> (Λ, Ψ), as Example07:124-125 reads them with `npzread`."""
    pv, pe = kl_paths(root_fname, data_dir)
    return np.load(pv).astype(np.float64).ravel(), np.asfortranarray(np.load(pe).astype(np.float64))


def save_greal(g, root_fname: str, data_dir: str = "data") -> str:
    """Example02:46 / Example04:100: `data/$root_fname.greal.npz`, one realization on the mesh nodes."""
    path = os.path.join(data_dir, f"{root_fname}.greal.npz")
    _write(path, np.asarray(g, dtype=np.float64))
    return path
