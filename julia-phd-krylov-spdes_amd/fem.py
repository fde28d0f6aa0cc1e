"""Host-side set-up that feeds the Schur-PCG hot path (boundary producer).

In the reference all of this runs once per realization on the host (Julia) and hands
arrays-of-SparseMatrixCSC plus index maps to the operators. It is NOT the hot path and
has no device kernels here either; it exists so that tests, `bench.py` and `smoke()` have
blocks of exactly the reference's shape to feed through the C ABI.

Citations are relative to /root/reference. "EPDD.jl" = Fem/EllipticPdeDomainDecomposition.jl.

Conventions (differences from the reference are layout only):
  * indices are 0-based here (the reference is 1-based Julia); `-1` means "absent";
  * the reference's `Dict{Int,Int}` maps are flat integer arrays
    (`gather_idx[d][l_Γd] = l_Γ` replaces `ind_Γd_Γ2l[d]`, EPDD.jl:186-191);
  * domains are numbered 0..ndom-1; `node_owner` keeps the reference's coding shifted by
    nothing for the special values: -1 = on Γ, -2 = Dirichlet, d>=0 = interior of d
    (reference: -1 / 0 / d>=1, EPDD.jl:43-46);
  * sparse blocks are scipy CSR. The symmetric blocks (A, A_II, A_ΓΓ) have identical
    CSR and CSC arrays; `A_IΓ` (n_I x n_Γd) is kept in CSR, i.e. the CSC arrays of its
    transpose `A_ΓI`.

Deviations from the reference that are not layout (SURVEY.md N2, §2 Mesh.jl row):
  * mesh = structured triangulation of the unit square (TriangleMesh is unavailable);
  * partition = element boxes (mpmetis is unavailable);
  * interior solves in set-up (`assemble_local_schurs`, `get_schur_rhs`,
    `get_subdomain_solutions`) use a sparse direct factorisation (scipy SuperLU) where
    the reference uses `IterativeSolvers.cg` to reltol 1e-9 / sqrt(eps).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Union

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

Coeff = Union[np.ndarray, Callable[[np.ndarray, np.ndarray], np.ndarray]]


# --------------------------------------------------------------------------------------
# Mesh and partition (substitutes for Fem/Mesh.jl:21-31 get_mesh and :169-195 mesh_partition)
# --------------------------------------------------------------------------------------
@dataclass
class Mesh:
    cells: np.ndarray           # (3, nel) int64, 0-based, counter-clockwise
    points: np.ndarray          # (2, nnode) float64
    point_marker: np.ndarray    # (nnode,) int64, 1 = Dirichlet boundary node
    cell_neighbors: np.ndarray  # (3, nel) int64, neighbour across the edge opposite vertex j, -1 = boundary
    N: int                      # nodes per side


def get_mesh(N: int) -> Mesh:
    """Structured P1 triangulation of the unit square with N x N nodes.

    Stands in for `get_mesh(tentative_nnode)` (Fem/Mesh.jl:21-31), which calls Triangle.
    Same output fields as the TriMesh the reference consumes (`cell`, `point`,
    `point_marker`, `cell_neighbor`); every boundary node is Dirichlet as in the
    reference's `point_marker`.
    """
    if N < 3:
        raise ValueError("need N >= 3")
    xs = np.linspace(0.0, 1.0, N)
    X, Y = np.meshgrid(xs, xs, indexing="xy")          # node id = j*N + i, x = xs[i], y = xs[j]
    points = np.stack([X.ravel(), Y.ravel()]).astype(np.float64)
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="xy")
    marker = ((ii == 0) | (ii == N - 1) | (jj == 0) | (jj == N - 1)).astype(np.int64).ravel()

    nc = N - 1
    ci, cj = np.meshgrid(np.arange(nc), np.arange(nc), indexing="xy")
    ci, cj = ci.ravel(), cj.ravel()                    # cell id c = cj*nc + ci
    n00 = cj * N + ci
    n10, n01, n11 = n00 + 1, n00 + N, n00 + N + 1
    nel = 2 * nc * nc
    cells = np.empty((3, nel), dtype=np.int64)
    cells[:, 0::2] = np.stack([n00, n10, n11])         # T0 of each cell
    cells[:, 1::2] = np.stack([n00, n11, n01])         # T1 of each cell
    c = cj * nc + ci
    nb = np.full((3, nel), -1, dtype=np.int64)
    # T0 = (n00, n10, n11): opposite n00 -> right cell's T1; n10 -> own T1; n11 -> lower cell's T1
    nb[0, 0::2] = np.where(ci + 1 < nc, 2 * (c + 1) + 1, -1)
    nb[1, 0::2] = 2 * c + 1
    nb[2, 0::2] = np.where(cj > 0, 2 * (c - nc) + 1, -1)
    # T1 = (n00, n11, n01): opposite n00 -> upper cell's T0; n11 -> left cell's T0; n01 -> own T0
    nb[0, 1::2] = np.where(cj + 1 < nc, 2 * (c + nc), -1)
    nb[1, 1::2] = np.where(ci > 0, 2 * (c - 1), -1)
    nb[2, 1::2] = 2 * c
    return Mesh(cells, points, marker, nb, N)


def mesh_partition(mesh: Mesh, px: int, py: int):
    """Element-box partition into px x py subdomains; returns (epart, npart), 0-based.

    Stands in for `mesh_partition(cells, ndom)` (Fem/Mesh.jl:169-195, mpmetis -contig).
    `npart[node]` is the domain of one element that owns the node, which is all
    `set_subdomains` needs (it reads npart only for nodes off the interface, EPDD.jl:168-174).
    """
    N = mesh.N
    nc = N - 1
    nel = mesh.cells.shape[1]
    c = np.arange(nel) // 2
    ci, cj = c % nc, c // nc
    bx = np.minimum(ci * px // nc, px - 1)
    by = np.minimum(cj * py // nc, py - 1)
    epart = (by * px + bx).astype(np.int64)
    npart = np.full(N * N, -1, dtype=np.int64)
    # last writer wins; any owner is valid for nodes off Γ
    for k in range(3):
        npart[mesh.cells[k]] = epart
    return epart, npart


# --------------------------------------------------------------------------------------
# Dirichlet index maps (Fem/BoundaryConditions.jl:35-57)
# --------------------------------------------------------------------------------------
@dataclass
class DirichletInds:
    dirichlet_g2l: np.ndarray       # (nnode,) -1 where not Dirichlet
    not_dirichlet_g2l: np.ndarray   # (nnode,) -1 where Dirichlet
    dirichlet_l2g: np.ndarray
    not_dirichlet_l2g: np.ndarray


def get_dirichlet_inds(points: np.ndarray, point_marker: np.ndarray) -> DirichletInds:
    """`get_dirichlet_inds` (Fem/BoundaryConditions.jl:35-57): ascending-node numbering of both sets."""
    nnode = points.shape[1]
    is_d = point_marker.ravel() == 1
    d_l2g = np.flatnonzero(is_d).astype(np.int64)
    nd_l2g = np.flatnonzero(~is_d).astype(np.int64)
    d_g2l = np.full(nnode, -1, dtype=np.int64)
    nd_g2l = np.full(nnode, -1, dtype=np.int64)
    d_g2l[d_l2g] = np.arange(d_l2g.size)
    nd_g2l[nd_l2g] = np.arange(nd_l2g.size)
    return DirichletInds(d_g2l, nd_g2l, d_l2g, nd_l2g)


def append_bc(dinds: DirichletInds, u_no_dirichlet, points, uexact):
    """`append_bc` (Fem/BoundaryConditions.jl:94-115)."""
    u = np.empty(points.shape[1])
    g = dinds.dirichlet_l2g
    u[g] = _eval(uexact, points[0, g], points[1, g])
    u[dinds.not_dirichlet_l2g] = u_no_dirichlet
    return u


def _eval(fn, x, y):
    out = fn(x, y)
    return np.broadcast_to(np.asarray(out, dtype=np.float64), np.shape(x)).astype(np.float64)


def _first_unique(a: np.ndarray) -> np.ndarray:
    """Unique values of `a` in order of first occurrence."""
    _, first = np.unique(a, return_index=True)
    return a[np.sort(first)]


# --------------------------------------------------------------------------------------
# set_subdomains (EPDD.jl:86-193)
# --------------------------------------------------------------------------------------
@dataclass
class Subdomains:
    ndom: int
    node_owner: np.ndarray              # (nnode,) -1 Γ, -2 Dirichlet, d interior
    node_Γ: np.ndarray                  # Γ-local -> global node (first-encounter order)
    node_Γ_cnt: np.ndarray              # (n_Γ,) number of subdomains sharing each Γ node
    node_Γd: List[np.ndarray]           # per domain: Γd-local -> global node (first-encounter order)
    node_Id: List[np.ndarray]           # per domain: I-local -> global node (ascending)
    gather_idx: List[np.ndarray]        # per domain: Γd-local -> Γ-local (flat ind_Γd_Γ2l)
    ind_Γ_g2l: np.ndarray               # (nnode,) global -> Γ-local or -1
    ind_I_g2l: np.ndarray               # (nnode,) global -> I-local in its owner domain or -1
    elemd: List[np.ndarray]             # elements of each domain (ascending)

    @property
    def n_Γ(self) -> int:
        return int(self.node_Γ.size)

    @property
    def n_Γd(self) -> List[int]:
        return [int(a.size) for a in self.node_Γd]

    @property
    def n_Id(self) -> List[int]:
        return [int(a.size) for a in self.node_Id]


def set_subdomains(cells, cell_neighbors, epart, npart, dirichlet_g2l) -> Subdomains:
    """`set_subdomains` (EPDD.jl:86-193).

    Γ = non-Dirichlet nodes shared by two edge-neighbouring elements of different
    subdomains (:125-152). Γ and every Γ_d are numbered by first encounter in the
    element loop (`for iel`, `for j in 1:3`, `for node in iel_cell`, :114-156);
    interiors are numbered by ascending node id within their `npart` owner (:167-181).
    """
    nel = cells.shape[1]
    nnode = int(cells.max()) + 1
    ndom = int(epart.max()) + 1
    is_dir = dirichlet_g2l >= 0

    # candidate events in reference loop order: (iel, j) with a neighbour in another domain
    jel = cell_neighbors                                    # (3, nel)
    valid = jel >= 0
    other = np.zeros_like(valid)
    other[valid] = epart[jel[valid]] != np.broadcast_to(epart, jel.shape)[valid]
    ev_j, ev_iel = np.nonzero(other)                        # row-major: sorted by j then iel
    order = np.lexsort((ev_j, ev_iel))                      # sort by iel, then j
    ev_iel, ev_j = ev_iel[order], ev_j[order]
    ev_jel = jel[ev_j, ev_iel]
    # for every event, nodes of iel (in cell order) that also belong to jel and are not Dirichlet
    icell = cells[:, ev_iel]                                # (3, nev)
    jcell = cells[:, ev_jel]
    shared = (icell[:, None, :] == jcell[None, :, :]).any(axis=1)   # (3, nev)
    shared &= ~is_dir[icell]
    k_idx, e_idx = np.nonzero(shared)
    seq = np.lexsort((k_idx, e_idx))                        # event order, then vertex order
    cand_nodes = icell[k_idx[seq], e_idx[seq]]
    cand_dom = epart[ev_iel[e_idx[seq]]]

    node_Γ = _first_unique(cand_nodes) if cand_nodes.size else np.empty(0, np.int64)
    ind_Γ_g2l = np.full(nnode, -1, dtype=np.int64)
    ind_Γ_g2l[node_Γ] = np.arange(node_Γ.size)

    node_owner = np.full(nnode, -3, dtype=np.int64)
    node_owner[is_dir] = -2
    node_owner[node_Γ] = -1

    node_Γd, gather_idx = [], []
    node_Γ_cnt = np.zeros(node_Γ.size, dtype=np.int64)
    for d in range(ndom):
        nd = cand_nodes[cand_dom == d]
        nd = _first_unique(nd) if nd.size else np.empty(0, np.int64)
        node_Γd.append(nd.astype(np.int64))
        g = ind_Γ_g2l[nd]
        gather_idx.append(g.astype(np.int64))
        node_Γ_cnt[g] += 1

    free_int = np.flatnonzero(node_owner == -3)
    node_owner[free_int] = npart[free_int]
    node_Id, ind_I_g2l = [], np.full(nnode, -1, dtype=np.int64)
    for d in range(ndom):
        nid = free_int[npart[free_int] == d]
        node_Id.append(nid.astype(np.int64))
        ind_I_g2l[nid] = np.arange(nid.size)

    elemd = [np.flatnonzero(epart == d).astype(np.int64) for d in range(ndom)]
    return Subdomains(ndom, node_owner, node_Γ.astype(np.int64), node_Γ_cnt, node_Γd, node_Id,
                      gather_idx, ind_Γ_g2l, ind_I_g2l, elemd)


# --------------------------------------------------------------------------------------
# Element kernels shared by the assemblies
# --------------------------------------------------------------------------------------
def _element_terms(cells, points, coeff: Coeff, f, uexact):
    """Per-element quantities, evaluated in the reference's operation order.

    Δa = (a1+a2+a3)/3 (EPDD.jl:260-269); shoelace terms (:272-277); Area (:280);
    ΔKij = Δa*(Δyi*Δyj + Δxi*Δxj)/4/Area (:294); Δb_i = (2f_i+f_j+f_k)*Area/12 (:340-349).
    """
    x = points[0][cells]            # (3, nel)
    y = points[1][cells]
    if callable(coeff):
        a = _eval(coeff, x, y)
    else:
        a = np.asarray(coeff, dtype=np.float64)[cells]
    Δa = np.zeros(cells.shape[1])
    for j in range(3):
        Δa = Δa + a[j]
    Δa = Δa / 3.0
    G, Area = _element_geometry(x, y)
    K = np.empty((3, 3, cells.shape[1]))
    for i in range(3):
        for j in range(3):
            K[i, j] = Δa * G[i, j] / 4 / Area
    fv = _eval(f, x, y)
    b = np.empty((3, cells.shape[1]))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        b[i] = (2 * fv[i] + fv[j] + fv[k]) * Area / 12
    ue = _eval(uexact, x, y)
    return K, b, ue


def _element_geometry(x, y):
    """Shoelace terms (EPDD.jl:272-277), G_ij = Δy_i*Δy_j + Δx_i*Δx_j (the coefficient-free factor of ΔK_ij) and Area (:280)."""
    Δx = np.stack([x[2] - x[1], x[0] - x[2], x[1] - x[0]])
    Δy = np.stack([y[1] - y[2], y[2] - y[0], y[0] - y[1]])
    Area = (Δx[2] * Δy[1] - Δx[1] * Δy[2]) / 2.0
    G = np.empty((3, 3, x.shape[1]))
    for i in range(3):
        for j in range(3):
            G[i, j] = Δy[i] * Δy[j] + Δx[i] * Δx[j]
    return G, Area


def _segment_sums(v, starts):
    """Sum of every segment v[starts[k]:starts[k+1]] taken strictly left to right, ((v0 + v1) + v2) + ... — the order
    in which Julia's `sparse(I,J,V)` combines duplicates and `b[k] += Δ` accumulates. (`np.add.reduceat` is NOT that:
    it adds the first term to the sum of the others.)"""
    ends = np.append(starts[1:], v.size)
    out = v[starts].copy()
    length = ends - starts
    for p in range(1, int(length.max()) if length.size else 0):
        m = length > p
        out[m] = out[m] + v[starts[m] + p]
    return out


def _coo_to_csr(I, J, V, shape, seq=None) -> sp.csr_matrix:
    """`sparse(I,J,V,m,n)`: duplicates are summed in order of occurrence (deterministic)."""
    if I.size == 0:
        return sp.csr_matrix(shape, dtype=np.float64)
    if seq is None:
        seq = np.arange(I.size)
    order = np.lexsort((seq, J, I))
    I, J, V = I[order], J[order], V[order]
    new = np.ones(I.size, dtype=bool)
    new[1:] = (I[1:] != I[:-1]) | (J[1:] != J[:-1])
    starts = np.flatnonzero(new)
    vals = _segment_sums(V, starts)
    rows, cols = I[starts], J[starts]
    indptr = np.zeros(shape[0] + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    indptr = np.cumsum(indptr)
    m = sp.csr_matrix((vals, cols.astype(np.int64), indptr), shape=shape)
    m.has_sorted_indices = True
    return m


def _accumulate(n, idx, vals, seq):
    """b[idx] += vals applied in `seq` order (sequential accumulation per entry)."""
    out = np.zeros(n)
    if idx.size:
        order = np.lexsort((seq, idx))
        i, v = idx[order], vals[order]
        new = np.ones(i.size, dtype=bool)
        new[1:] = i[1:] != i[:-1]
        starts = np.flatnonzero(new)
        out[i[starts]] = _segment_sums(v, starts)
    return out


# --------------------------------------------------------------------------------------
# Full-system assembly (Fem/EllipticPde.jl:60-157 function coeff, :187-275 nodal coeff)
# --------------------------------------------------------------------------------------
def do_isotropic_elliptic_assembly(cells, points, dinds: DirichletInds, point_marker,
                                   a: Coeff, f, uexact):
    """Full Galerkin system on the non-Dirichlet nodes: returns (A csr, b)."""
    K, be, ue = _element_terms(cells, points, a, f, uexact)
    nel = cells.shape[1]
    n = dinds.not_dirichlet_l2g.size
    is_dir = point_marker.ravel()[cells] == 1       # (3, nel)
    loc = dinds.not_dirichlet_g2l[cells]            # -1 on Dirichlet
    I, J, V, S = [], [], [], []
    bi, bv, bs = [], [], []
    el = np.arange(nel)
    for i in range(3):
        for j in range(3):
            both = ~is_dir[i] & ~is_dir[j]
            I.append(loc[i][both]); J.append(loc[j][both]); V.append(K[i, j][both])
            S.append(el[both] * 9 + i * 3 + j)
            lift = is_dir[i] & ~is_dir[j]
            bi.append(loc[j][lift]); bv.append(-(ue[i][lift] * K[i, j][lift]))
            bs.append(el[lift] * 12 + i * 3 + j)
    for i in range(3):
        free = ~is_dir[i]
        bi.append(loc[i][free]); bv.append(be[i][free]); bs.append(el[free] * 12 + 9 + i)
    A = _coo_to_csr(np.concatenate(I), np.concatenate(J), np.concatenate(V), (n, n), np.concatenate(S))
    b = _accumulate(n, np.concatenate(bi), np.concatenate(bv), np.concatenate(bs))
    return A, b


# --------------------------------------------------------------------------------------
# prepare_local_schurs / prepare_global_schur (EPDD.jl:389-546 / 212-369)
# --------------------------------------------------------------------------------------
def _triplets(cells, sub: Subdomains, local: bool):
    """Index side of the element loop (EPDD.jl:283-350 / 459-527): for every block the COO (row, col) pairs and, for
    every pair, its sequence code s = 12*element + 3*i + j (stiffness term ΔK_ij, also the Dirichlet lifting when it
    lands in a right-hand side) or 12*element + 9 + i (load term Δb_i). The code is both the reference's order of
    accumulation and the address of the value, so the numeric side (host: `_values`, device: `AssemblyPlan`) needs
    nothing else."""
    nel = cells.shape[1]
    owner = sub.node_owner[cells]                   # (3, nel)
    el = np.arange(nel)
    gΓ = sub.ind_Γ_g2l[cells]
    gI = sub.ind_I_g2l[cells]
    # Γ_d-local index of every (vertex, element): only meaningful where owner == -1
    gΓd = np.full(cells.shape, -1, dtype=np.int64)
    tmp = np.full(sub.node_owner.size, -1, dtype=np.int64)
    for d in range(sub.ndom):
        tmp[sub.node_Γd[d]] = np.arange(sub.node_Γd[d].size)
        e = sub.elemd[d]
        gΓd[:, e] = tmp[cells[:, e]]
        tmp[sub.node_Γd[d]] = -1
    cat = np.concatenate
    out = dict(II=[], IΓ=[], ΓΓ=[], bI=[], bΓ=None, ΓΓ_glob=None)
    bΓ_i, bΓ_s = [], []
    ΓΓ_glob = ([], [], [])
    for d in range(sub.ndom):
        e = sub.elemd[d]
        ow = owner[:, e]
        gId, gΓe, gΓde, ele = gI[:, e], gΓ[:, e], gΓd[:, e], el[e]
        II = ([], [], []); IΓ = ([], [], []); ΓΓ = ([], [], [])
        bI = ([], [])
        for i in range(3):
            for j in range(3):
                s = ele * 12 + i * 3 + j
                oi, oj = ow[i], ow[j]
                m = (oi == -1) & (oj == -1)
                if local:
                    ΓΓ[0].append(gΓde[i][m]); ΓΓ[1].append(gΓde[j][m]); ΓΓ[2].append(s[m])
                else:
                    ΓΓ_glob[0].append(gΓe[i][m]); ΓΓ_glob[1].append(gΓe[j][m]); ΓΓ_glob[2].append(s[m])
                m = (oi >= 0) & (oj >= 0)
                II[0].append(gId[i][m]); II[1].append(gId[j][m]); II[2].append(s[m])
                m = (oi >= 0) & (oj == -1)
                IΓ[0].append(gId[i][m]); IΓ[1].append((gΓde if local else gΓe)[j][m]); IΓ[2].append(s[m])
                # Dirichlet lifting (EPDD.jl:322-331 / 498-507): b[j] -= ΔK_ij * uexact(node i)
                m = (oi == -2) & (oj == -1)
                bΓ_i.append(gΓe[j][m]); bΓ_s.append(s[m])
                m = (oi == -2) & (oj >= 0)
                bI[0].append(gId[j][m]); bI[1].append(s[m])
        for i in range(3):
            s = ele * 12 + 9 + i
            m = ow[i] == -1
            bΓ_i.append(gΓe[i][m]); bΓ_s.append(s[m])
            m = ow[i] >= 0
            bI[0].append(gId[i][m]); bI[1].append(s[m])
        out["II"].append(tuple(cat(v) for v in II))
        out["IΓ"].append(tuple(cat(v) for v in IΓ))
        if local:
            out["ΓΓ"].append(tuple(cat(v) for v in ΓΓ))
        out["bI"].append(tuple(cat(v) for v in bI))
    out["bΓ"] = (cat(bΓ_i), cat(bΓ_s))
    if not local:
        out["ΓΓ_glob"] = tuple(cat(v) for v in ΓΓ_glob)
    return out


def _values(seq, K, be, ue, rhs: bool):
    """Value of every contribution from its sequence code: ΔK_ij; in a right-hand side -(ΔK_ij * uexact_i) or Δb_i."""
    e, c = seq // 12, seq % 12
    if not rhs:
        return K.reshape(9, -1)[c, e]
    lift = c < 9
    cl = np.where(lift, c, 0)
    v = -(K.reshape(9, -1)[cl, e] * ue[cl // 3, e])
    return np.where(lift, v, be[np.where(lift, 0, c - 9), e])


def _prepare(cells, points, epart, sub: Subdomains, coeff, f, uexact, local: bool):
    K, be, ue = _element_terms(cells, points, coeff, f, uexact)
    T = _triplets(cells, sub, local)
    n_Γ = sub.n_Γ
    A_II, A_IΓ, A_ΓΓ_parts, b_Id = [], [], [], []
    for d in range(sub.ndom):
        nI, nΓd = sub.node_Id[d].size, sub.node_Γd[d].size
        I, J, S = T["II"][d]
        A_II.append(_coo_to_csr(I, J, _values(S, K, be, ue, False), (nI, nI), S))
        I, J, S = T["IΓ"][d]
        A_IΓ.append(_coo_to_csr(I, J, _values(S, K, be, ue, False), (nI, nΓd if local else n_Γ), S))
        if local:
            I, J, S = T["ΓΓ"][d]
            A_ΓΓ_parts.append(_coo_to_csr(I, J, _values(S, K, be, ue, False), (nΓd, nΓd), S))
        I, S = T["bI"][d]
        b_Id.append(_accumulate(nI, I, _values(S, K, be, ue, True), S))
    I, S = T["bΓ"]
    b_Γ = _accumulate(n_Γ, I, _values(S, K, be, ue, True), S)
    if local:
        return A_II, A_IΓ, A_ΓΓ_parts, b_Id, b_Γ
    I, J, S = T["ΓΓ_glob"]
    A_ΓΓ = _coo_to_csr(I, J, _values(S, K, be, ue, False), (n_Γ, n_Γ), S)
    return A_II, A_IΓ, A_ΓΓ, b_Id, b_Γ


def prepare_local_schurs(cells, points, epart, sub: Subdomains, coeff: Coeff, f, uexact):
    """`prepare_local_schurs` (EPDD.jl:389-546): (A_IIdd, A_IΓdd, A_ΓΓdd, b_Id, b_Γ), Γ_d-local columns."""
    return _prepare(cells, points, epart, sub, coeff, f, uexact, local=True)


def prepare_global_schur(cells, points, epart, sub: Subdomains, coeff: Coeff, f, uexact):
    """`prepare_global_schur` (EPDD.jl:212-369): (A_IId, A_IΓd, A_ΓΓ, b_Id, b_Γ), Γ-global columns."""
    return _prepare(cells, points, epart, sub, coeff, f, uexact, local=False)


@dataclass
class GammaGatherMap:
    """A_ΓΓ = Σ_d R_d' A_ΓΓdd R_d as a gather: the CSC pattern of the global block (symmetric, so also its CSR arrays) and,
    for every stored entry e, the flat indices `src[e, :]` of its local contributions in ascending subdomain order (padding
    points past the end, at an appended zero). `values(v)` sums them in that fixed order — numpy or torch CUDA alike, no
    scatter-add — so device-assembled values (`api.AssemblyPlan.run`) refresh A_ΓΓ_t without the host (Example07:416).
    The sum is grouped by subdomain, `prepare_global_schur` groups by element: the two agree to rounding, not bit for bit."""
    n: int
    indptr: np.ndarray
    indices: np.ndarray
    src: np.ndarray        # (nnz, width) int64
    n_src: int             # length of the flat value array the indices point into

    def values(self, v):
        if type(v).__module__.startswith("torch"):
            import torch
            src = getattr(self, "_src_t", None)
            if src is None or src.device != v.device:
                src = self._src_t = torch.as_tensor(self.src, device=v.device)
            ext = torch.cat([v[:self.n_src], v.new_zeros(1)])
            out = ext[src[:, 0]]
            for c in range(1, src.shape[1]):
                out = out + ext[src[:, c]]
            return out
        ext = np.concatenate([np.asarray(v, dtype=np.float64)[:self.n_src], [0.0]])
        out = ext[self.src[:, 0]]
        for c in range(1, self.src.shape[1]):
            out = out + ext[self.src[:, c]]
        return out

    def matrix(self, v) -> sp.csc_matrix:
        return sp.csc_matrix((np.asarray(self.values(v)), self.indices, self.indptr), shape=(self.n, self.n))


def gamma_gather_map(patterns, gather_idx, n_Γ: int, offsets=None) -> GammaGatherMap:
    """`patterns`: per subdomain A_ΓΓdd (scipy, Γ_d-local, symmetric) or its (indptr, indices, shape); `offsets`: where each
    subdomain's nzval starts in the flat value array (default: the blocks back to back; `AssemblyPlan.layout["ΓΓ"]` offsets
    make `values` read the output of an assembly run directly)."""
    rows, cols, flat, dom = [], [], [], []
    off = 0
    n_src = 0
    for d, pat in enumerate(patterns):
        if sp.issparse(pat):
            m = sp.csr_matrix(pat)
            indptr, indices = m.indptr, m.indices
        else:
            indptr, indices = pat[0], pat[1]
        o = off if offsets is None else int(offsets[d])
        nnz = int(indptr[-1])
        r = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
        g = np.asarray(gather_idx[d], dtype=np.int64)
        rows.append(g[r]); cols.append(g[np.asarray(indices, dtype=np.int64)])
        flat.append(o + np.arange(nnz, dtype=np.int64)); dom.append(np.full(nnz, d, dtype=np.int64))
        off += nnz
        n_src = max(n_src, o + nnz)
    rows, cols, flat, dom = (np.concatenate(a) for a in (rows, cols, flat, dom))
    order = np.lexsort((flat, dom, rows, cols))                 # CSC order: column, row; then subdomain
    rows, cols, flat = rows[order], cols[order], flat[order]
    new = np.ones(rows.size, dtype=bool)
    new[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    entry = np.cumsum(new) - 1
    nE = int(entry[-1]) + 1 if entry.size else 0
    first = np.flatnonzero(new)
    rank = np.arange(rows.size) - first[entry]
    width = int(rank.max()) + 1 if rank.size else 1
    src = np.full((nE, width), n_src, dtype=np.int64)
    src[entry, rank] = flat
    indptr = np.zeros(n_Γ + 1, dtype=np.int64)
    np.add.at(indptr, cols[first] + 1, 1)
    return GammaGatherMap(n_Γ, np.cumsum(indptr), rows[first].astype(np.int64), src, n_src)


@dataclass
class AssemblyPlan:
    """The index half of `prepare_local_schurs` (EPDD.jl:389-546) for a FIXED mesh, partition, `f` and `uexact`: what
    Example07's realization loop (:162-171) recomputes for every coefficient draw although only `a` changes.

    Output entries, in this order: the stored values of A_IIdd[0..ndom), A_IΓdd[0..ndom), A_ΓΓdd[0..ndom) — the `nzval`
    of Julia's CSC matrices, which is also what `mi_schur_matfree_*create` / `_set_values` take — then b_Id[0..ndom), b_Γ. Entry k is the sum, in the reference's
    element order, of the contributions `ccode[cptr[k]:cptr[k+1]]`; a contribution code is 12*element + 3*i + j
    (ΔK_ij = Δa*G_ij/4/Area; in a right-hand side: -(ΔK_ij*ue_i)) or 12*element + 9 + i (Δb_i, coefficient-free).
    `api.AssemblyPlan(ctx, plan)` runs it on the GPU; `blocks(values)` rebuilds the scipy matrices on the host."""
    cells: np.ndarray
    G: np.ndarray          # (9, nel)
    area: np.ndarray       # (nel,)
    ue: np.ndarray         # (3, nel)
    be: np.ndarray         # (3, nel)
    cptr: np.ndarray
    ccode: np.ndarray
    n_matrix_entries: int
    layout: dict           # name -> list of (offset, count) per subdomain (b_Γ: single tuple)
    patterns: dict         # name -> list of (indptr, indices, shape)
    n_node: int

    @property
    def n_entries(self) -> int:
        return self.cptr.size - 1

    def blocks(self, values: np.ndarray):
        """(A_IIdd, A_IΓdd, A_ΓΓdd, b_Id, b_Γ) from a flat value array, as `prepare_local_schurs` returns them."""
        values = np.asarray(values, dtype=np.float64)
        out = []
        for name in ("II", "IΓ", "ΓΓ"):
            mats = []
            for (off, cnt), (indptr, indices, shape) in zip(self.layout[name], self.patterns[name]):
                if name == "IΓ":
                    m = sp.csc_matrix((values[off:off + cnt].copy(), indices, indptr), shape=shape).tocsr()
                else:
                    m = sp.csr_matrix((values[off:off + cnt].copy(), indices, indptr), shape=shape)
                m.has_sorted_indices = True
                mats.append(m)
            out.append(mats)
        out.append([values[off:off + cnt].copy() for off, cnt in self.layout["bI"]])
        off, cnt = self.layout["bΓ"]
        out.append(values[off:off + cnt].copy())
        return tuple(out)


def make_assembly_plan(cells, points, epart, sub: Subdomains, f, uexact) -> AssemblyPlan:
    x, y = points[0][cells], points[1][cells]
    G, Area = _element_geometry(x, y)
    fv = _eval(f, x, y)
    be = np.empty((3, cells.shape[1]))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        be[i] = (2 * fv[i] + fv[j] + fv[k]) * Area / 12
    ue = _eval(uexact, x, y)
    T = _triplets(cells, sub, local=True)
    counts, codes = [], []
    layout = dict(II=[], IΓ=[], ΓΓ=[], bI=[], bΓ=None)
    patterns = dict(II=[], IΓ=[], ΓΓ=[])
    off = 0
    for name in ("II", "IΓ", "ΓΓ"):
        for d in range(sub.ndom):
            I, J, S = T[name][d]
            nI, nΓd = sub.node_Id[d].size, sub.node_Γd[d].size
            shape = dict(II=(nI, nI), IΓ=(nI, nΓd), ΓΓ=(nΓd, nΓd))[name]
            if name == "IΓ":
                I, J = J, I            # A_IΓdd is stored by COLUMN (the CSC arrays the C ABI takes = CSR of A_ΓIdd)
            order = np.lexsort((S, J, I))
            I, J, S = I[order], J[order], S[order]
            new = np.ones(I.size, dtype=bool)
            new[1:] = (I[1:] != I[:-1]) | (J[1:] != J[:-1])
            starts = np.flatnonzero(new)
            indptr = np.zeros((shape[1] if name == "IΓ" else shape[0]) + 1, dtype=np.int64)
            np.add.at(indptr, I[starts] + 1, 1)
            patterns[name].append((np.cumsum(indptr), J[starts].astype(np.int64), shape))
            counts.append(np.diff(np.append(starts, I.size)))
            codes.append(S)
            layout[name].append((off, starts.size))
            off += starts.size
    n_matrix = off
    rhs = [(T["bI"][d], sub.node_Id[d].size) for d in range(sub.ndom)] + [(T["bΓ"], sub.n_Γ)]
    for k, ((idx, S), n) in enumerate(rhs):
        order = np.lexsort((S, idx))
        counts.append(np.bincount(idx, minlength=n).astype(np.int64))
        codes.append(S[order])
        if k < sub.ndom:
            layout["bI"].append((off, n))
        else:
            layout["bΓ"] = (off, n)
        off += n
    cptr = np.zeros(off + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts), out=cptr[1:])
    return AssemblyPlan(np.ascontiguousarray(cells, dtype=np.int64), np.ascontiguousarray(G.reshape(9, -1)),
                        np.ascontiguousarray(Area), np.ascontiguousarray(ue), np.ascontiguousarray(be), cptr,
                        np.concatenate(codes).astype(np.int64), n_matrix, layout, patterns, int(points.shape[1]))


# --------------------------------------------------------------------------------------
# Row-owned plan of the full-system assembly (Fem/EllipticPde.jl:187-275, in place :291-377)
# --------------------------------------------------------------------------------------
FA_ROWS = 256        # csrc/full_assembly_plan.hpp: rows of a row block (one thread each)
FA_SEG = 4096        # stored entries of a row block (one workgroup's LDS segment)
FA_DIR = 0xFFFF      # "Dirichlet" in a 16-bit row position


@dataclass
class FullAssemblyPlan:
    """The index half of `do_isotropic_elliptic_assembly` / `update_isotropic_elliptic_assembly!` (EllipticPde.jl:187-275 /
    :291-377) for a FIXED mesh, Dirichlet maps, `f` and `uexact`: what Example06's realization loop redoes for every draw
    although only `a` changes. The python mirror of csrc/full_assembly_plan.hpp, array for array.

    Row-owned: free node r is row r of A; everything in row r and in b[r] comes from the elements incident to that node, in
    ascending element number (the order of `sparse(I,J,V)` and `b[k] +=`). `inc_code[inc_ptr[r]:inc_ptr[r+1]]` = 4 e + i
    (the row's node is vertex i of element e); `inc_pos` holds, for the two other vertices in ascending local index, the
    position of their column in the row (low / high 16 bits) or FA_DIR: a Dirichlet vertex, whose pair is a lifting term of
    b[r]. `blk_row`: row blocks of at most FA_ROWS rows and FA_SEG stored entries, never a split row.
    `api.FullAssemblyPlan(ctx, plan)` runs it on the GPU."""
    cells: np.ndarray      # (3, nel) int64, 0-based
    points: np.ndarray     # (2, n_node)
    point_marker: np.ndarray
    ue: np.ndarray         # (3, nel)
    be: np.ndarray         # (3, nel)
    node_row: np.ndarray
    rowptr: np.ndarray
    colidx: np.ndarray
    diag_pos: np.ndarray
    inc_ptr: np.ndarray
    inc_code: np.ndarray
    inc_pos: np.ndarray
    blk_row: np.ndarray

    @property
    def n(self) -> int:
        return self.rowptr.size - 1

    @property
    def nnz(self) -> int:
        return self.colidx.size

    @property
    def n_node(self) -> int:
        return self.points.shape[1]

    @property
    def n_entries(self) -> int:
        return self.nnz + self.n

    def bytes(self) -> int:
        """Device bytes of the plan: index arrays, ue, be, points (full_assembly_plan.hpp `Plan::bytes`)."""
        nel = self.cells.shape[1]
        ints = (3 * nel + self.rowptr.size + self.diag_pos.size + self.inc_ptr.size + self.inc_code.size + self.inc_pos.size
                + self.blk_row.size)
        return 4 * ints + 8 * (6 * nel + 2 * self.n_node)

    def system(self, values, b):
        """(A csr, b) from the CSR values and the right-hand side of a run."""
        A = sp.csr_matrix((np.array(values, dtype=np.float64), self.colidx.copy(), self.rowptr.copy()), shape=(self.n, self.n))
        A.has_sorted_indices = True
        return A, np.array(b, dtype=np.float64)

    def run(self, a):
        """(values, b): numpy restatement of `k_assemble_full`. Row r walks its incidence list; per incidence the element's
        terms are recomputed in the order of `_element_terms`, and each ΔK_ij is added to the row's entry or, for a Dirichlet
        vertex j, as -(ue_j ΔK_ij) to b[r] (j ascending), then Δb_i. Every accumulator starts at -0.0, the exact additive
        identity, so the first contribution is an assignment in effect (`_segment_sums`)."""
        a = np.asarray(a, dtype=np.float64)
        n, nel = self.n, self.cells.shape[1]
        vals = np.full(self.nnz, -0.0)
        b = np.full(n, -0.0)
        cnt = np.diff(self.inc_ptr)
        for p in range(int(cnt.max()) if n else 0):
            r = np.flatnonzero(cnt > p)
            q = self.inc_ptr[r] + p
            e, i = self.inc_code[q] >> 2, self.inc_code[q] & 3
            c = self.cells[:, e]
            x, y, av = self.points[0][c], self.points[1][c], a[c]
            Δa = ((av[0] + av[1]) + av[2]) / 3.0
            Δx = np.stack([x[2] - x[1], x[0] - x[2], x[1] - x[0]])
            Δy = np.stack([y[1] - y[2], y[2] - y[0], y[0] - y[1]])
            Area = (Δx[2] * Δy[1] - Δx[1] * Δy[2]) / 2.0
            k = np.arange(r.size)
            Δxi, Δyi = Δx[i, k], Δy[i, k]
            slot = np.zeros(r.size, dtype=np.int64)
            for j in range(3):
                K = Δa * (Δyi * Δy[j] + Δxi * Δx[j]) / 4 / Area
                own = i == j
                pos = np.where(own, self.diag_pos[r], (self.inc_pos[q] >> (16 * slot)) & 0xFFFF)
                slot = slot + ~own
                lift = pos == FA_DIR
                t = self.rowptr[r[~lift]] + pos[~lift]
                vals[t] = vals[t] + K[~lift]
                b[r[lift]] = b[r[lift]] + -(self.ue[j, e[lift]] * K[lift])
            b[r] = b[r] + self.be[i, e]
        b[cnt == 0] = 0.0
        return vals, b

    def as_block_plan(self) -> AssemblyPlan:
        """The same system as a generic `AssemblyPlan`: entries = the CSR values of A followed by b, one contribution code per
        term (12 e + 3 i + j, or 12 e + 9 + i). `oracle.run_assembly_plan` and `api.AssemblyPlan` execute it unchanged: the
        independent cross-check of `run` and of the device kernel."""
        nel = self.cells.shape[1]
        x, y = self.points[0][self.cells], self.points[1][self.cells]
        G, Area = _element_geometry(x, y)
        row = np.repeat(np.arange(self.n), np.diff(self.inc_ptr))
        e, i = self.inc_code >> 2, self.inc_code & 3
        target, code = [], []
        slot = np.zeros(row.size, dtype=np.int64)
        for j in range(3):
            own = i == j
            pos = np.where(own, self.diag_pos[row], (self.inc_pos >> (16 * slot)) & 0xFFFF)
            slot = slot + ~own
            lift = pos == FA_DIR
            target.append(np.where(lift, self.nnz + row, self.rowptr[row] + np.where(lift, 0, pos)))
            code.append(np.where(lift, 12 * e + 3 * j + i, 12 * e + 3 * i + j))
        target.append(self.nnz + row)
        code.append(12 * e + 9 + i)
        target, code = np.concatenate(target), np.concatenate(code)
        order = np.lexsort((code, target))
        cptr = np.zeros(self.n_entries + 1, dtype=np.int64)
        np.cumsum(np.bincount(target, minlength=self.n_entries), out=cptr[1:])
        return AssemblyPlan(np.ascontiguousarray(self.cells, dtype=np.int64), np.ascontiguousarray(G.reshape(9, -1)),
                            np.ascontiguousarray(Area), np.ascontiguousarray(self.ue), np.ascontiguousarray(self.be), cptr,
                            code[order].astype(np.int64), self.nnz, {}, {}, self.n_node)


def make_full_assembly_plan(cells, points, dinds: DirichletInds, point_marker, f, uexact) -> FullAssemblyPlan:
    """Python mirror of `mi::fap::make_plan` (csrc/full_assembly_plan.hpp); `f` and `uexact` enter through `be` and `ue`
    only. Refusals raise ValueError with the text of the C++ plan."""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    points = np.ascontiguousarray(points, dtype=np.float64)
    marker = np.ascontiguousarray(point_marker, dtype=np.int64).ravel()
    nel, n_node = cells.shape[1], points.shape[1]
    if nel < 1:
        raise ValueError(f"full assembly plan: nel = {nel} elements (at least 1 expected)")
    if 4 * nel >= 2 ** 31:
        raise ValueError(f"full assembly plan: nel = {nel} elements: 4 nel = {4 * nel} does not fit 31 bits")
    bad = np.argwhere(((cells < 0) | (cells >= n_node)).T)
    if bad.size:
        e, i = bad[0]
        raise ValueError(f"full assembly plan: element {e}, vertex {i}: node {cells[i, e]} is outside the mesh")
    rep = (cells[0] == cells[1]) | (cells[1] == cells[2]) | (cells[0] == cells[2])
    x, y = points[0][cells], points[1][cells]
    _, Area = _element_geometry(x, y)
    flat = ~((Area != 0.0) & np.isfinite(Area))
    first = np.flatnonzero(rep | flat)
    if first.size:
        e = int(first[0])
        if rep[e]:
            c = cells[:, e]
            raise ValueError(f"full assembly plan: element {e} lists node {c[0] if c[0] in (c[1], c[2]) else c[1]} twice")
        raise ValueError(f"full assembly plan: element {e} has zero area (or coordinates that are not finite)")
    node_row = np.full(n_node, -1, dtype=np.int64)
    free = np.flatnonzero(marker != 1)
    node_row[free] = np.arange(free.size)
    if not np.array_equal(node_row, dinds.not_dirichlet_g2l):
        raise ValueError("full assembly plan: dinds.not_dirichlet_g2l is not the ascending numbering of the nodes with point_marker != 1")
    n = free.size
    loc = node_row[cells]                                      # (3, nel)
    el = np.arange(nel)
    rows = np.concatenate([loc[i] for i in range(3)])
    codes = np.concatenate([4 * el + i for i in range(3)])
    keep = rows >= 0
    rows, codes = rows[keep], codes[keep]
    order = np.lexsort((codes, rows))
    rows, codes = rows[order], codes[order]
    inc_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=inc_ptr[1:])
    e, i = codes >> 2, codes & 3
    cols = loc[:, e]                                           # (3, ninc): columns of the three vertices, -1 = Dirichlet
    key = np.unique(np.concatenate([(rows * n + cols[j])[cols[j] >= 0] for j in range(3)])) if rows.size else np.zeros(0, dtype=np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=rowptr[1:])
    length = np.diff(rowptr)
    if n and length.max() > FA_SEG:
        r = int(np.argmax(length > FA_SEG))
        raise ValueError(f"full assembly plan: row {r} has {length[r]} stored entries, more than FA_SEG = {FA_SEG}")
    colidx = key % max(n, 1)
    diag_pos = np.searchsorted(key, np.arange(n) * n + np.arange(n)) - rowptr[:-1]
    inc_pos = np.zeros(rows.size, dtype=np.int64)
    slot = np.zeros(rows.size, dtype=np.int64)
    for j in range(3):
        other = i != j
        pos = np.where(cols[j] >= 0, np.searchsorted(key, rows * n + np.maximum(cols[j], 0)) - rowptr[rows], FA_DIR)
        inc_pos = inc_pos | np.where(other, pos << (16 * slot), 0)
        slot = slot + other
    blk = [0]
    while blk[-1] < n:
        r0 = blk[-1]
        blk.append(int(min(r0 + FA_ROWS, np.searchsorted(rowptr, rowptr[r0] + FA_SEG, side="right") - 1)))
    fv = _eval(f, x, y)
    be = np.empty((3, nel))
    for v in range(3):
        j, k = (v + 1) % 3, (v + 2) % 3
        be[v] = (2 * fv[v] + fv[j] + fv[k]) * Area / 12
    ue = _eval(uexact, x, y)
    return FullAssemblyPlan(cells, points, marker, np.ascontiguousarray(ue), np.ascontiguousarray(be), node_row, rowptr, colidx,
                            diag_pos, inc_ptr, codes, inc_pos, np.asarray(blk, dtype=np.int64))


# --------------------------------------------------------------------------------------
# Interior solves and assembled local Schur complements
# --------------------------------------------------------------------------------------
class InteriorSolver:
    """Host-side A_II^{-1} (sparse direct). Stands in for the reference's
    `IterativeSolvers.cg(A_II, rhs; Pl=AMG, reltol)` (EPDD.jl:648-650) and is what
    BASELINE.json's north_star calls "the host-side sparse Cholesky"."""

    def __init__(self, A_II: sp.spmatrix):
        self.n = A_II.shape[0]
        self.lu = spla.splu(sp.csc_matrix(A_II), permc_spec="MMD_AT_PLUS_A",
                            diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))

    def __call__(self, rhs: np.ndarray) -> np.ndarray:
        return self.lu.solve(np.ascontiguousarray(rhs, dtype=np.float64))


class LazySolvers:
    """`solvers[d]`: the InteriorSolver of subdomain d, factorised on first use (d outside [lo, hi) -> None)."""

    def __init__(self, A_II, lo, hi):
        self._A, self._lo, self._hi, self._f = A_II, lo, hi, {}

    def __len__(self):
        return len(self._A)

    def __getitem__(self, d):
        if isinstance(d, slice):
            return [self[k] for k in range(*d.indices(len(self)))]
        if d < 0:
            d += len(self._A)
        if not (self._lo <= d < self._hi):
            return None
        if d not in self._f:
            self._f[d] = InteriorSolver(self._A[d])
        return self._f[d]

    def __iter__(self):
        return (self[d] for d in range(len(self._A)))


def _bfs_levels_from_interface(A_II: sp.csr_matrix, seeds: np.ndarray):
    """Breadth-first levels of the graph of A_II starting from `seeds`; nodes that are not
    connected to the seeds are left out (they cannot influence the Schur complement)."""
    n = A_II.shape[0]
    level = np.full(n, -1, dtype=np.int64)
    level[seeds] = 0
    frontier, levels = np.asarray(seeds, dtype=np.int64), []
    indptr, indices = A_II.indptr, A_II.indices
    while frontier.size:
        levels.append(frontier)
        starts, ends = indptr[frontier], indptr[frontier + 1]
        cnt = ends - starts
        idx = np.repeat(starts - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(cnt.sum())
        nb = np.unique(indices[idx])
        nb = nb[level[nb] < 0]
        level[nb] = len(levels)
        frontier = nb
    return levels


def _dense_device():
    """Where the dense level recursion runs: the GPU through torch when one is visible (set-up
    only — rocBLAS/rocSOLVER library calls, not part of the hot path), else torch on the CPU,
    else numpy. scipy.linalg is avoided: its bundled OpenBLAS stalls for ~0.5 s per small
    Cholesky when 8+ threads spin inside a container."""
    try:
        import torch
    except ImportError:
        return None, None
    import os
    if torch.cuda.is_available() and not os.environ.get("MI355_SETUP_ON_CPU"):
        return torch, torch.device("cuda")
    return torch, torch.device("cpu")


def local_schur_by_level_elimination(A_II, A_IΓ, A_ΓΓ, b_I=None):
    """Dense S_d = A_ΓΓ - A_IΓ' A_II^{-1} A_IΓ by exact block elimination; with `b_I` also the condensed
    right-hand side A_IΓ' A_II^{-1} b_I (what `get_schur_rhs` subtracts from b_Γ, EPDD.jl:853-861), returned as
    (S_d, w_d).

    The interior is split into breadth-first levels L_0, L_1, ... grown from the interior nodes
    adjacent to Γ_d; A_II is block tridiagonal in that ordering, so eliminating from the deepest
    level towards Γ_d is the recursion T_m = A_mm, T_k = A_kk - A_{k+1,k}' T_{k+1}^{-1} A_{k+1,k}
    (and g_m = b_m, g_k = b_k - A_{k+1,k}' T_{k+1}^{-1} g_{k+1}), and S_d = A_ΓΓ - A_{0Γ}' T_0^{-1} A_{0Γ},
    w_d = A_{0Γ}' T_0^{-1} g_0. Every step is dense Cholesky + triangular solve + product (BLAS-3), which is
    far faster than n_Γd sparse triangular solves with 124 k unknowns. Interior nodes not connected to Γ_d
    cannot influence either result and are left out.
    """
    A_II = sp.csr_matrix(A_II)
    A_IΓ = sp.csr_matrix(A_IΓ)
    S = np.asarray(sp.csr_matrix(A_ΓΓ).todense(), dtype=np.float64)
    seeds = np.flatnonzero(np.diff(A_IΓ.indptr) > 0)
    if seeds.size == 0:
        return S if b_I is None else (S, np.zeros(S.shape[0]))
    levels = _bfs_levels_from_interface(A_II, seeds)
    perm = np.concatenate(levels)
    off = np.concatenate(([0], np.cumsum([l.size for l in levels])))
    Ap = sp.csr_matrix(A_II[perm][:, perm])
    torch, dev = _dense_device()

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if torch is not None else a

    def blk(i, j):
        return to_dev(Ap[off[i]:off[i + 1], off[j]:off[j + 1]].toarray())

    if torch is not None:
        chol = torch.linalg.cholesky
        def trsm(c, b):
            return torch.linalg.solve_triangular(c, b, upper=False)
    else:
        import scipy.linalg as sla
        chol = np.linalg.cholesky
        def trsm(c, b):
            return sla.solve_triangular(c, b, lower=True, check_finite=False)

    bp = None if b_I is None else np.asarray(b_I, dtype=np.float64)[perm]
    m = len(levels) - 1
    T = blk(m, m)
    g = None if bp is None else to_dev(bp[off[m]:off[m + 1]].reshape(-1, 1))
    for k in range(m - 1, -1, -1):
        c = chol(T)
        C = blk(k + 1, k)
        Y = trsm(c, C if g is None else (torch.cat([C, g], 1) if torch is not None else np.hstack([C, g])))
        Yc = Y if g is None else Y[:, :-1]
        T = blk(k, k) - Yc.T @ Yc
        if g is not None:
            g = to_dev(bp[off[k]:off[k + 1]].reshape(-1, 1)) - Yc.T @ Y[:, -1:]
    c = chol(T)
    B = to_dev(A_IΓ[levels[0]].toarray())
    Y = trsm(c, B if g is None else (torch.cat([B, g], 1) if torch is not None else np.hstack([B, g])))
    Yc = Y if g is None else Y[:, :-1]
    YtY = Yc.T @ Yc
    S -= YtY.cpu().numpy() if torch is not None else YtY
    if g is None:
        return S
    w = Yc.T @ Y[:, -1:]
    return S, (w.cpu().numpy() if torch is not None else w).ravel()


def assemble_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, solvers: Optional[Sequence["InteriorSolver"]] = None,
                          method: str = "levels", chunk: int = 256, b_Id=None):
    """`assemble_local_schurs` (EPDD.jl:667-695): dense S_d = A_ΓΓd - A_IΓd' A_IId^{-1} A_IΓd.

    The reference applies `apply_local_schur` (interior CG, reltol 1e-9) to every unit vector and
    keeps the upper triangle (`Symmetric(Array(map))`, :692). Here the blocks come from an exact
    direct elimination (`method="levels"`, see local_schur_by_level_elimination) or from multi-RHS
    SuperLU solves (`method="solves"`, slow; kept as the cross-check), and are symmetrised the
    same way. Returns column-major (Fortran-order) arrays like Julia's `Array`; with `b_Id` (levels only)
    also the list of condensed right-hand sides A_IΓd' A_IId^{-1} b_Id.
    """
    out, ws = [], []
    for d in range(len(A_IIdd)):
        n = A_ΓΓdd[d].shape[0]
        if method == "levels":
            res = local_schur_by_level_elimination(A_IIdd[d], A_IΓdd[d], A_ΓΓdd[d], None if b_Id is None else b_Id[d])
            S = res if b_Id is None else res[0]
            if b_Id is not None:
                ws.append(res[1])
        else:
            solve = solvers[d] if solvers is not None else InteriorSolver(A_IIdd[d])
            S = np.asarray(A_ΓΓdd[d].todense(), dtype=np.float64)
            AIΓ = sp.csc_matrix(A_IΓdd[d])
            AΓI = sp.csr_matrix(A_IΓdd[d].T)
            for c0 in range(0, n, chunk):
                c1 = min(n, c0 + chunk)
                V = solve(AIΓ[:, c0:c1].toarray())
                S[:, c0:c1] -= AΓI @ V
        S = np.triu(S) + np.triu(S, 1).T
        out.append(np.asfortranarray(S))
    return out if b_Id is None else (out, ws)


def prepare_neumann_neumann_schur_precond(Sd: Sequence[np.ndarray]):
    """`prepare_neumann_neumann_schur_precond(Sd_local_mat, ...)` (EPDD.jl:1201-1220):
    ΠS_d = pinv(S_d, rtol = sqrt(eps(Float64))) — SVD-based, singular values <= rtol*σ_max dropped.
    Runs on the GPU through torch when one is visible (set-up only), else numpy; same definition."""
    rtol = float(np.sqrt(np.finfo(np.float64).eps))
    torch, dev = _dense_device()
    out = []
    for S in Sd:
        S = np.asarray(S, dtype=np.float64)
        if torch is not None and dev.type == "cuda" and S.shape[0] > 0:
            P = torch.linalg.pinv(torch.from_numpy(np.ascontiguousarray(S)).to(dev), rtol=rtol, hermitian=False).cpu().numpy()
        else:
            P = np.linalg.pinv(S, rcond=rtol)
        out.append(np.asfortranarray(P))
    return out


def prepare_neumann_neumann_induced_precond(A_IIdd, A_IΓdd, A_ΓΓdd):
    """The numeric half of `prepare_neumann_neumann_induced_precond` (EPDD.jl:2305-2353): per subdomain the dense
    `Sd_mat = Array(Sd)` of `apply_local_schur` (:2322-2338) and ΠS_d = pinv(Sd_mat, rtol = sqrt(eps)) (:2339). The
    blocks come from `assemble_local_schurs` (exact elimination in place of the reference's interior CG at reltol 1e-12)
    and `prepare_neumann_neumann_schur_precond`; the Cholesky factors of :2340 are the kept levels of the device set-up
    plan. Returns the list of ΠS_d, column-major."""
    return prepare_neumann_neumann_schur_precond(assemble_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd))


def prepare_lorasc_precond(S, A_ΓΓ, nvec: int = 25, ε: float = 0.01, eigs=None):
    """The low-rank correction of `prepare_lorasc_precond`, its `low_rank_correction = :exact` branch (EPDD.jl:1541-1617),
    on the host: the `nvec` least dominant generalized eigenpairs S e = σ A_ΓΓ e by a dense `scipy.linalg.eigh(S, A_ΓΓ)`
    in place of `KrylovKit.geneigsolve(..., nvec, :SR, isposdef=true)` (:1546-1549) — both leave `E' A_ΓΓ E = I`.
    `S` is the dense Schur complement or a callable x -> S x. Returns `(E[:, :nev], Σ[:nev])`.

    The selection (:1587-1610): pairs in ascending σ; the leading ones with σ < ε are counted as nev and their Σ[k]
    becomes (ε - σ)/σ, the count stops at the first σ >= ε; nev == 0 -> nev = nvec (with untransformed Σ), as the
    reference falls back; nev == nvec is kept (the reference only warns). ε <= 0 gives no correction (:1612-1615).

    `eigs`: an optional callable nvec -> (Σ, E) that supplies the pairs instead of the dense `eigh` (the device form:
    `lambda k: api.geneigsolve(S_op, A_ΓΓ_op, chol_A_ΓΓ, k, "SR", krylovdim=2 * k)[:2]`); `S` is then not touched and may
    be None. The selection above is applied to what it returns."""
    n = A_ΓΓ.shape[0]
    if eigs is not None:
        if ε <= 0:
            return np.empty((n, 0)), np.empty(0)
        nvec = min(int(nvec), n)
        Σ, E = eigs(nvec)
        Σ, E = np.array(Σ, dtype=np.float64), np.asarray(E, dtype=np.float64)
        if Σ.shape != (nvec,) or E.shape != (n, nvec):
            raise ValueError(f"eigs({nvec}) returned shapes {Σ.shape}, {E.shape}; ({nvec},) and ({n}, {nvec}) expected")
        return _lorasc_select(Σ, E, nvec, ε)
    A = A_ΓΓ.toarray() if sp.issparse(A_ΓΓ) else np.asarray(A_ΓΓ, dtype=np.float64)
    n = A.shape[0]
    if ε <= 0:
        return np.empty((n, 0)), np.empty(0)
    if callable(S):
        S = np.column_stack([S(e) for e in np.eye(n)])
    S = np.asarray(S, dtype=np.float64)
    nvec = min(int(nvec), n)
    import scipy.linalg as sla
    Σ, E = sla.eigh((S + S.T) / 2, (A + A.T) / 2, subset_by_index=[0, nvec - 1])
    return _lorasc_select(Σ, E, nvec, ε)


def _lorasc_select(Σ, E, nvec: int, ε: float):
    """EPDD.jl:1587-1610 on the nvec pairs (see prepare_lorasc_precond)."""
    order = np.argsort(Σ, kind="stable")
    Σ, E = Σ[order].copy(), E[:, order]
    nev = 0
    for k in range(nvec):
        if Σ[k] < ε:
            Σ[k] = (ε - Σ[k]) / Σ[k]
            nev += 1
        else:
            break
    if nev == 0:
        nev = nvec
    return np.asfortranarray(E[:, :nev]), Σ[:nev]


def lorasc_maps(sub: Subdomains, dinds: DirichletInds):
    """Rows of A (`not_dirichlet_inds_g2l`, EPDD.jl:1924, 1930) of every subdomain's interior nodes and of the Γ nodes."""
    g2l = dinds.not_dirichlet_g2l
    return [g2l[nodes] for nodes in sub.node_Id], g2l[sub.node_Γ]


# --------------------------------------------------------------------------------------
# Smoothed-aggregation AMG set-up (Preconditioners.AMGPreconditioner{SmoothedAggregation}, Example01:49-61)
# --------------------------------------------------------------------------------------
AMG_MAX_COARSE_ROWS = 4096   # the coarsest level is kept as a dense inverse: never above this many rows
AMG_STALL = 0.9              # aggregation that keeps >= 90 % of the rows has stalled


@dataclass
class AmgHierarchy:
    """What `prepare_amg_precond` hands to the device (`api.AMGPreconditioner`) and to the tests' restatement of the cycle.
    Level l < nlevels - 1 is smoothed and has a prolongator; the last level is solved by `coarse_inv`."""
    A: List[sp.csr_matrix]            # [nlevels] A_l, symmetric, sorted CSR
    P: List[sp.csr_matrix]            # [nlevels - 1] P_l, n_l x n_{l+1}, sorted CSR
    omega: List[float]                # [nlevels - 1] ω_l = 4 / (3 g_l)
    omega_over_d: List[np.ndarray]    # [nlevels - 1] ω_l / diag(A_l)
    coarse_inv: np.ndarray            # n_c x n_c, symmetric, column-major
    sizes: List[int]                  # [nlevels] n_l
    operator_complexity: float        # Σ_l nnz(A_l) / nnz(A_0)
    agg: Optional[List[np.ndarray]] = None   # [nlevels - 1] aggregate of every node of level l, 0-based (`amg_refresh`, the device set-up)

    @property
    def nlevels(self) -> int:
        return len(self.A)

    @property
    def operator_nnz(self) -> int:
        return int(sum(a.nnz for a in self.A))


def amg_aggregate(A: sp.csr_matrix) -> np.ndarray:
    """Standard aggregation on the strength graph "every off-diagonal non-zero" (symmetric strength, θ = 0), three passes,
    each over the nodes in ascending order: (1) a free node whose strong neighbours are all free seeds an aggregate and
    takes them in; (2) every remaining node joins the aggregate of its first neighbour (stored order) that pass 1
    aggregated; (3) a leftover becomes an aggregate together with its free neighbours. Returns agg[i], 0-based, dense."""
    n = A.shape[0]
    ptr, idx, val = A.indptr.tolist(), A.indices.tolist(), (A.data != 0).tolist()
    nbr = [[j for j, nz in zip(idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]) if nz and j != i] for i in range(n)]
    agg = [-1] * n
    na = 0
    for i in range(n):
        if agg[i] >= 0:
            continue
        nb = nbr[i]
        for j in nb:
            if agg[j] >= 0:
                break
        else:
            agg[i] = na
            for j in nb:
                agg[j] = na
            na += 1
    first = agg[:]
    for i in range(n):
        if agg[i] >= 0:
            continue
        for j in nbr[i]:
            if first[j] >= 0:
                agg[i] = first[j]
                break
    for i in range(n):
        if agg[i] >= 0:
            continue
        agg[i] = na
        for j in nbr[i]:
            if agg[j] < 0:
                agg[j] = na
        na += 1
    return np.asarray(agg, dtype=np.int64)


def _amg_sorted_csr(M) -> sp.csr_matrix:
    M = sp.csr_matrix(M)
    M.sum_duplicates()
    M.sort_indices()
    return M


def prepare_amg_precond(A, max_levels: int = 10, max_coarse: int = 256) -> AmgHierarchy:
    """Smoothed aggregation on the host, once per matrix — the set-up of the reference's
    `AMGPreconditioner{SmoothedAggregation}(A)` (Example01:49-61; AlgebraicMultigrid.jl's defaults: symmetric strength
    with θ = 0, standard aggregation, the constant near-null-space). Per level, with d = diag(A_l):

        T[i, agg(i)] = 1 / sqrt(|agg|)                       tentative prolongator
        P_l = (I - ω_l D^-1 A_l) T,  ω_l = 4 / (3 g_l),      g_l = max_i Σ_j |a_ij| / a_ii  (Gershgorin bound on ρ(D^-1 A_l):
                                                             no eigen-estimate, deterministic)
        A_{l+1} = P_l' A_l P_l, symmetrised as (M + M') / 2

    Coarsening stops at n_l <= max_coarse or at max_levels levels; the last level keeps the dense inverse of its
    symmetrised matrix, symmetrised too. `max_levels = 1` is the dense inverse of A itself. Raises ValueError when the
    aggregation stalls (n_{l+1} >= 0.9 n_l: a large level is never densified) and when the coarsest level would hold more
    than 4096 rows. The cycle that uses the hierarchy: one pre- and one post-sweep of Jacobi damped by ω_l."""
    A0 = _amg_sorted_csr(A)
    if A0.shape[0] != A0.shape[1] or A0.shape[0] == 0:
        raise ValueError("square, non-empty matrix expected")
    if max_levels < 1:
        raise ValueError(f"max_levels = {max_levels} (at least 1)")
    if not np.isfinite(A0.data).all():
        raise ValueError("the matrix holds a value that is not finite")
    As, Ps, om, owd, aggs = [A0], [], [], [], []
    while len(As) < max_levels and As[-1].shape[0] > max_coarse:
        Al = As[-1]
        n = Al.shape[0]
        d = Al.diagonal()
        if not (d > 0).all():
            raise ValueError(f"level {len(As) - 1}: a diagonal entry is not positive")
        agg = amg_aggregate(Al)
        nc = int(agg.max()) + 1
        if nc >= AMG_STALL * n:
            raise ValueError(f"level {len(As) - 1}: aggregation stalled, {n} rows -> {nc} aggregates "
                             f"(>= {AMG_STALL} n); the level is not densified")
        cnt = np.bincount(agg, minlength=nc).astype(np.float64)
        T = sp.csr_matrix((1.0 / np.sqrt(cnt[agg]), (np.arange(n), agg)), shape=(n, nc))
        g = float(np.max(np.asarray(abs(Al).sum(axis=1)).ravel() / d))
        w = 4.0 / (3.0 * g)
        wd = w / d
        P = _amg_sorted_csr(T - sp.diags(wd) @ (Al @ T))
        M = (P.T @ Al @ P).tocsr()
        As.append(_amg_sorted_csr((M + M.T) * 0.5))
        Ps.append(P); om.append(w); owd.append(wd); aggs.append(agg)
    nc = As[-1].shape[0]
    if nc > AMG_MAX_COARSE_ROWS:
        raise ValueError(f"the coarsest level holds {nc} rows, more than the {AMG_MAX_COARSE_ROWS} a dense inverse is kept for "
                         f"(max_levels = {max_levels}, max_coarse = {max_coarse})")
    Ac = As[-1].toarray()
    inv = np.linalg.inv((Ac + Ac.T) * 0.5)
    if not np.isfinite(inv).all():
        raise ValueError("the coarsest level is singular")
    inv = np.asfortranarray((inv + inv.T) * 0.5)
    nnz = [a.nnz for a in As]
    return AmgHierarchy(As, Ps, om, owd, inv, [a.shape[0] for a in As], float(sum(nnz)) / float(nnz[0]), aggs)


def _amg_ones(M) -> sp.csr_matrix:
    """the stored pattern of M as a matrix of ones (stored zeros are entries)"""
    M = sp.csr_matrix(M)
    return sp.csr_matrix((np.ones(M.indices.size), M.indices.copy(), M.indptr.copy()), shape=M.shape)


def _amg_embed(V, S) -> sp.csr_matrix:
    """The values of V on the stored pattern of S ⊇ pattern(V), zeros elsewhere; both sorted CSR."""
    V, S = _amg_sorted_csr(V), _amg_sorted_csr(S)
    key = lambda M: np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * M.shape[1] + M.indices
    kv, ks = key(V), key(S)
    pos = np.searchsorted(ks, kv)
    if kv.size and (pos.max(initial=0) >= ks.size or (ks[np.minimum(pos, ks.size - 1)] != kv).any()):
        raise ValueError("a computed entry lies outside the structural pattern")
    data = np.zeros(ks.size)
    data[pos] = V.data
    return sp.csr_matrix((data, S.indices.copy(), S.indptr.copy()), shape=S.shape)


def amg_refresh(H_or_aggs, A) -> AmgHierarchy:
    """The numeric chain of `prepare_amg_precond` for a new matrix `A` on FROZEN aggregates — `H_or_aggs`: a hierarchy with
    `.agg`, or the list of aggregate arrays itself (one per smoothed level, 0-based). The host restatement of the device
    set-up (`api.AMGPreconditioner(ctx, A, device_setup=True).set_values`): the same arithmetic as `prepare_amg_precond`,
    expression for expression, but on the STRUCTURAL patterns — P_l on pattern(T) ∪ pattern(A_l T), A_{l+1} on the pattern of
    the all-ones product P_l' A_l P_l — where scipy drops an entry whose value cancels to exactly zero. `amg_aggregate` sees a
    matrix only through `data != 0`, so for a matrix with the stored non-zeros of the one the aggregates came from, the
    result equals `prepare_amg_precond(A)` wherever that stores an entry (tests/test_amg_refresh_cpu.py); for any other
    matrix it is a valid hierarchy, but not the one a fresh set-up would build."""
    aggs = H_or_aggs.agg if isinstance(H_or_aggs, AmgHierarchy) else H_or_aggs
    if aggs is None:
        raise ValueError("the hierarchy carries no aggregates (built by hand, or before `agg` existed)")
    aggs = [np.asarray(a, dtype=np.int64).ravel() for a in aggs]
    A0 = _amg_sorted_csr(A)
    if A0.shape[0] != A0.shape[1] or A0.shape[0] == 0:
        raise ValueError("square, non-empty matrix expected")
    if not np.isfinite(A0.data).all():
        raise ValueError("the matrix holds a value that is not finite")
    As, Ps, om, owd = [A0], [], [], []
    for l, agg in enumerate(aggs):
        Al = As[-1]
        n = Al.shape[0]
        if agg.size != n:
            raise ValueError(f"level {l}: {agg.size} aggregate ids for {n} rows")
        d = Al.diagonal()
        if not (d > 0).all():
            raise ValueError(f"level {l}: a diagonal entry is not positive")
        nc = int(agg.max()) + 1
        cnt = np.bincount(agg, minlength=nc).astype(np.float64)
        if agg.min() < 0 or not (cnt > 0).all():
            raise ValueError(f"level {l}: a negative aggregate id or an empty aggregate")
        T = sp.csr_matrix((1.0 / np.sqrt(cnt[agg]), (np.arange(n), agg)), shape=(n, nc))
        g = float(np.max(np.asarray(abs(Al).sum(axis=1)).ravel() / d))
        w = 4.0 / (3.0 * g)
        wd = w / d
        T1, A1 = _amg_ones(T), _amg_ones(Al)
        P = _amg_embed(T - sp.diags(wd) @ (Al @ T), T1 + A1 @ T1)
        M = (P.T @ Al @ P).tocsr()
        P1 = _amg_ones(P)
        As.append(_amg_embed((M + M.T) * 0.5, sp.csr_matrix(P1.T) @ (A1 @ P1)))
        Ps.append(P); om.append(w); owd.append(wd)
    nc = As[-1].shape[0]
    if nc > AMG_MAX_COARSE_ROWS:
        raise ValueError(f"the coarsest level holds {nc} rows, more than the {AMG_MAX_COARSE_ROWS} a dense inverse is kept for")
    Ac = As[-1].toarray()
    inv = np.linalg.inv((Ac + Ac.T) * 0.5)
    if not np.isfinite(inv).all():
        raise ValueError("the coarsest level is singular")
    inv = np.asfortranarray((inv + inv.T) * 0.5)
    nnz = [a.nnz for a in As]
    return AmgHierarchy(As, Ps, om, owd, inv, [a.shape[0] for a in As], float(sum(nnz)) / float(nnz[0]), aggs)


def prepare_interior_amg(A_IIdd, max_levels: int = 10, max_coarse: int = 256):
    """The aggregates of the AMG `Pl` of the device interior CG (`api.MatrixFreeLocalSchurs.interior_amg`,
    `mi_schur_interior_amg`): `prepare_amg_precond` on the stacked block-diagonal matrix blockdiag(A_IIdd), for its
    aggregation alone — the numbers of the hierarchy are made on the device from the operator's own values. Returns
    (sizes, aggs): the level sizes (sizes[0] = Σ_d n_Id) and one 0-based aggregate array per smoothed level, over the stacked
    nodes. `amg_aggregate` looks at neighbours only, so every block gets exactly the aggregates it would get alone
    (renumbered); the stop rule `n_l <= max_coarse` counts stacked rows. Raises the ValueErrors of `prepare_amg_precond`
    (no interior node at all, max_levels < 1, a diagonal entry that is not positive, a stalled aggregation, a coarsest level
    above 4096 rows)."""
    blocks = [sp.csr_matrix(A) for A in A_IIdd]
    if not blocks or sum(A.shape[0] for A in blocks) == 0:
        raise ValueError("square, non-empty matrix expected")
    H = prepare_amg_precond(sp.block_diag(blocks, format="csr"), max_levels=max_levels, max_coarse=max_coarse)
    return list(H.sizes), [np.asarray(a, dtype=np.int64) for a in H.agg]


def get_schur_rhs(b_Id, A_IId, A_IΓd, b_Γ, gather_idx=None, solvers=None):
    """`get_schur_rhs` (EPDD.jl:798-821 global columns; :835-864 local columns + scatter)."""
    b = np.array(b_Γ, dtype=np.float64, copy=True)
    for d in range(len(b_Id)):
        solve = solvers[d] if solvers is not None else InteriorSolver(A_IId[d])
        w = A_IΓd[d].T @ solve(b_Id[d])
        if gather_idx is None:
            b -= w
        else:
            b[gather_idx[d]] -= w
    return b


def get_subdomain_solutions(u_Γ, A_IId, A_IΓd_global, b_Id, solvers=None):
    """`get_subdomain_solutions` (EPDD.jl:1014-1025): u_I = A_II^{-1}(b_I - A_IΓ u_Γ)."""
    out = []
    for d in range(len(b_Id)):
        solve = solvers[d] if solvers is not None else InteriorSolver(A_IId[d])
        out.append(solve(b_Id[d] - A_IΓd_global[d] @ u_Γ))
    return out


def merge_subdomain_solutions(u_Γ, u_Id, sub: Subdomains, dinds: DirichletInds, uexact, points):
    """`merge_subdomain_solutions` (EPDD.jl:1040-1070)."""
    u = np.empty(points.shape[1])
    u[sub.node_Γ] = u_Γ
    for d in range(sub.ndom):
        u[sub.node_Id[d]] = u_Id[d]
    g = dinds.dirichlet_l2g
    u[g] = _eval(uexact, points[0, g], points[1, g])
    return u


# --------------------------------------------------------------------------------------
# Synthetic lognormal coefficient (semantics of
# `draw!` Fem/KarhunenLoeveDomainDecomposition.jl:1026-1044: g = Σ sqrt(Λ_α) ξ_α Ψ[:,α])
# --------------------------------------------------------------------------------------
@dataclass
class SyntheticKL:
    Λ: np.ndarray       # (m,)
    Ψ: np.ndarray       # (nnode, m)


def synthetic_kl(points, m_side: int = 8, L: float = 0.1, sig2: float = 1.0) -> SyntheticKL:
    """Separable cosine modes Ψ_{kl} = cos(kπx)cos(lπy), Λ_{kl} ∝ exp(-(k²+l²)π²L²/4),
    scaled so that Σ Λ = sig2; m = m_side² modes ordered by decreasing Λ (ties: k then l)."""
    ks, ls = np.meshgrid(np.arange(m_side), np.arange(m_side), indexing="ij")
    ks, ls = ks.ravel(), ls.ravel()
    lam = np.exp(-(ks ** 2 + ls ** 2) * np.pi ** 2 * L ** 2 / 4)
    order = np.lexsort((ls, ks, -lam))
    ks, ls, lam = ks[order], ls[order], lam[order]
    lam = lam * (sig2 / lam.sum())
    x, y = points
    Ψ = np.cos(np.pi * x[:, None] * ks[None, :]) * np.cos(np.pi * y[:, None] * ls[None, :])
    return SyntheticKL(lam, Ψ)


def draw(kl: SyntheticKL, rng: np.random.Generator):
    """`draw!`: ξ ~ N(0, I); g = Σ_α sqrt(Λ_α) ξ_α Ψ[:,α] accumulated mode by mode."""
    ξ = rng.standard_normal(kl.Λ.size)
    g = np.zeros(kl.Ψ.shape[0])
    for α in range(kl.Λ.size):
        g += (np.sqrt(kl.Λ[α]) * ξ[α]) * kl.Ψ[:, α]
    return ξ, g


def set_field(Λ, Ψ, ξ):
    """The loop of `draw` without the random numbers (`set!`, KLDD.jl:1150-1164; Samplers.jl:81-87):
    g = Σ_α (sqrt(Λ_α) ξ_α) Ψ[:, α], mode by mode from zero. A non-finite ξ gives IEEE results, not an error."""
    Λ, Ψ, ξ = np.asarray(Λ, dtype=np.float64), np.asarray(Ψ, dtype=np.float64), np.asarray(ξ, dtype=np.float64)
    g = np.zeros(Ψ.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for α in range(Λ.size):
            g += (np.sqrt(Λ[α]) * ξ[α]) * Ψ[:, α]
    return g


def draw_dd_field(nnode: int, Λ, Φ, Φd, inds_l2gd, ξ):
    """The field of `draw(mesh, Λ, Φ, Φd, inds_l2gd)` (KLDD.jl:850-883) for a given ξ, in the reference's own loop order:
    g[inode] += sqrt(Λ_γ) ξ_γ Φ[ind(idom, α), γ] Φd[idom][i, α] over (idom, α, γ), then g ./= cnt. Ψ is never formed."""
    Λ, Φ, ξ = np.asarray(Λ, dtype=np.float64), np.asarray(Φ, dtype=np.float64), np.asarray(ξ, dtype=np.float64)
    g = np.zeros(nnode)
    cnt = np.zeros(nnode, dtype=np.int64)
    c = np.sqrt(Λ) * ξ
    off = 0
    for idom, l2g in enumerate(inds_l2gd):
        cnt[l2g] += 1
        P = np.asarray(Φd[idom], dtype=np.float64)
        for α in range(P.shape[1]):
            for γ in range(Λ.size):
                g[l2g] += c[γ] * Φ[off + α, γ] * P[:, α]
        off += P.shape[1]
    return g / cnt


def get_kl_coordinates(g, Λ, Φ, M):
    """`get_kl_coordinates(g, Λ, Φ, M)` (KLDD.jl:1109-1124): ξ_α = Σ_i Φ[i, α] (M g)[i] / sqrt(Λ_α), every term divided,
    rows ascending."""
    Λ, Φ = np.asarray(Λ, dtype=np.float64), np.asarray(Φ, dtype=np.float64)
    w = M @ np.asarray(g, dtype=np.float64)
    ξ = np.zeros(Λ.size)
    for α in range(Λ.size):
        terms = Φ[:, α] * w / np.sqrt(Λ[α])
        for t in terms:
            ξ[α] += t
    return ξ


# --------------------------------------------------------------------------------------
# Karhunen-Loève layer, host side (Fem/KarhunenLoeve.jl, Fem/KarhunenLoeveDomainDecomposition.jl = "KLDD.jl",
# Fem/KarhunenLoeveDomainDecompositionHelper.jl, Fem/Covariances.jl). The covariance-heavy parts run on the device
# (api.solve_kl, api.solve_local_kl, api.do_global_mass_covariance_reduced_assembly); what follows is index work, the small
# dense eigenproblem and the projection. Subdomains are numbered from 0, maps are flat arrays with -1 for "absent".
# --------------------------------------------------------------------------------------
COV_MODELS = ("SExp", "Exp")     # the names of get_root_filename (KarhunenLoeveDomainDecompositionHelper.jl:54)


def cov(model: str, x1, y1, x2, y2, sig2: float = 1.0, L: float = 0.1):
    """`cov_sexp` (Covariances.jl:23-28) and the exponential model, written as the reference writes them (numpy, elementwise)."""
    r2 = (x1 - x2) ** 2 + (y1 - y2) ** 2
    if model == "SExp":
        return sig2 * np.exp(-r2 / L ** 2)
    if model == "Exp":
        return sig2 * np.exp(-np.sqrt(r2) / L)
    raise ValueError(f"model = {model!r}: one of {COV_MODELS} expected")


def _element_areas(cells, points):
    x, y = points[0][cells], points[1][cells]
    return _element_geometry(x, y)[1]


def _mass_triplets(cells, Area):
    """Element mass matrices Area/12 [2 1 1; 1 2 1; 1 1 2] in the push! order of EllipticPde.jl:442-459 (element, i, j)."""
    nel = cells.shape[1]
    I = np.repeat(cells.T[:, :, None], 3, axis=2).reshape(-1)            # cells[i, el] for (el, i, j)
    J = np.repeat(cells.T[:, None, :], 3, axis=1).reshape(-1)            # cells[j, el]
    V = np.where(np.eye(3, dtype=bool)[None], (Area / 6.0)[:, None, None], (Area / 12.0)[:, None, None]).reshape(-1)
    assert I.size == 9 * nel
    return I.astype(np.int64), J.astype(np.int64), V


def get_mass_matrix(cells, points) -> sp.csr_matrix:
    """`get_mass_matrix(cells, points)` (EllipticPde.jl:412-466): the consistent P1 mass matrix, M[i, j] = ∫ ϕ_i ϕ_j."""
    I, J, V = _mass_triplets(cells, _element_areas(cells, points))
    n = points.shape[1]
    return _coo_to_csr(I, J, V, (n, n))


def kl_set_subdomain(cells, points, epart, idom: int):
    """`set_subdomain(cells, points, epart, idom)` (KLDD.jl:40-80) -> (inds_l2g, inds_g2l, elems, center): ALL nodes of the
    subdomain's elements in first-seen order (element by element, vertex by vertex); the centre is their mean."""
    elems = np.flatnonzero(np.asarray(epart) == idom).astype(np.int64)
    inds_l2g = _first_unique(cells[:, elems].T.reshape(-1)).astype(np.int64)
    inds_g2l = np.full(points.shape[1], -1, dtype=np.int64)
    inds_g2l[inds_l2g] = np.arange(inds_l2g.size)
    center = np.zeros(2)
    for inode in inds_l2g:                                   # the reference's summation order (KLDD.jl:73-77)
        center[0] += points[0, inode]
        center[1] += points[1, inode]
    center /= inds_l2g.size
    return inds_l2g, inds_g2l, elems, center


def do_local_mass_assembly(cells, points, inds_g2l, elems) -> sp.csr_matrix:
    """`do_local_mass_assembly` (KLDD.jl:236-293): the mass matrix of one subdomain in its local numbering."""
    sub = cells[:, elems]
    I, J, V = _mass_triplets(inds_g2l[sub], _element_areas(sub, points))
    n = int((inds_g2l >= 0).sum())
    return _coo_to_csr(I, J, V, (n, n))


def kl_energy(cells, points, elems=None):
    """(Area, centre) as solve_kl integrates them (KarhunenLoeve.jl:145-165): the area of the elements and the mean over
    the elements of their centroids, accumulated vertex by vertex."""
    sub = cells if elems is None else cells[:, elems]
    Area = 0.0
    for a in _element_areas(sub, points):
        Area += a
    center = np.zeros(2)
    for el in range(sub.shape[1]):
        for r in range(3):
            center[0] += points[0, sub[r, el]] / 3
            center[1] += points[1, sub[r, el]] / 3
    center /= sub.shape[1]
    return float(Area), center


def kl_keep(λ, energy_expected: float):
    """The keep loop of KarhunenLoeve.jl:169-180 / KLDD.jl:706-717 -> (nvec, energy_achieved): positive eigenvalues, in the
    order given, until `energy_expected` is reached."""
    energy_achieved, nvec = 0.0, 0
    for λ_i in λ:
        if λ_i > 0:
            nvec += 1
            energy_achieved += float(λ_i)
        else:
            break
        if energy_achieved >= energy_expected:
            break
    return nvec, energy_achieved


def trim_and_order(Λ, Φ):
    """`trim_and_order` (KLDD.jl:1070-1077): drop the (leading, `eigen` is ascending) negative values, most dominant first."""
    Λ, Φ = np.asarray(Λ), np.asarray(Φ)
    neg_vals = int(np.sum(Λ < 0))
    return Λ[neg_vals:][::-1].copy(), Φ[:, neg_vals:][:, ::-1].copy()


def project_on_mesh(nnodes: int, Φ, elemsd, inds_l2gd, Φd):
    """`project_on_mesh` (KLDD.jl:920-959): Ψ[inode, imode] = (Σ_idom Σ_α Φ[ind(idom, α), imode] Φd[idom][i, α]) / cnt[inode],
    cnt the number of subdomains a node belongs to. Sums run in the reference's order (idom, then α, ascending)."""
    Φ = np.asarray(Φ)
    nmodes = Φ.shape[1]
    Ψ = np.zeros((nnodes, nmodes))
    cnt = np.zeros(nnodes, dtype=np.int64)
    off = 0
    for idom, l2g in enumerate(inds_l2gd):
        cnt[l2g] += 1
        md = Φd[idom].shape[1]
        for α in range(md):
            Ψ[l2g, :] += Φd[idom][:, α][:, None] * Φ[off + α, :][None, :]
        off += md
    return Ψ / cnt[:, None]


def solve_global_reduced_kl(nnode: int, K, energy_expected: float, elemsd, inds_l2gd, Φd, relative: float = 0.99, verbose: bool = True):
    """`solve_global_reduced_kl` (KLDD.jl:783-810): `eigen(Symmetric(K))` (the upper triangle), trim_and_order, the energy
    truncation, project_on_mesh -> (Λ[:nvec], Ψ)."""
    import scipy.linalg as sla
    Λ, Φ = sla.eigh(np.asarray(K), lower=False)
    Λ, Φ = trim_and_order(Λ, Φ)
    energy_expected *= relative
    energy_achieved, nvec = 0.0, 0
    for λ_i in Λ:
        energy_achieved += float(λ_i)
        nvec += 1
        if energy_achieved >= energy_expected:
            break
    Ψ = project_on_mesh(nnode, Φ[:, :nvec], elemsd, inds_l2gd, Φd)
    if verbose:
        print(f"{nvec}/{Λ.size} vectors kept for {energy_achieved / energy_expected * relative:.5f} relative energy")
    return Λ[:nvec], Ψ


@dataclass
class KLSubDomain:
    """The reference's `SubDomain` (returned by solve_local_kl, KLDD.jl:729-734) plus the local mass matrix it was solved with."""
    inds_g2l: np.ndarray      # (nnode,) local index of a mesh node, -1 outside the subdomain
    inds_l2g: np.ndarray      # (n_d,) mesh node of a local node, first-seen order
    elems: np.ndarray         # elements of the subdomain
    Φ: np.ndarray             # (n_d, nvec) kept local eigenfunctions, Φ' M Φ = I
    center: np.ndarray        # (2,)
    energy: float             # Area * cov(center, center)
    M: sp.csr_matrix          # do_local_mass_assembly
    λ: np.ndarray = None      # all nev local eigenvalues (what save_eigvals writes, KLDD.jl:680-684)


def suggest_parameters(nnode: int):
    """`suggest_parameters(nnode)` (KarhunenLoeveDomainDecompositionHelper.jl:35-41) -> (relative_local, relative_global)."""
    return (.9986, .995) if nnode <= 100_000 else (.9993, .995)


# --------------------------------------------------------------------------------------
# One-call problem builders used by tests, smoke() and bench.py
# --------------------------------------------------------------------------------------
@dataclass
class SchurProblem:
    mesh: Mesh
    dinds: DirichletInds
    sub: Subdomains
    epart: np.ndarray
    A_IIdd: list
    A_IΓdd: list
    A_ΓΓdd: list
    b_Id: list
    b_Γ: np.ndarray
    b_schur: np.ndarray
    Sd: Optional[list] = None       # dense local Schur complements, column-major
    ΠSd: Optional[list] = None      # their pseudo-inverses, column-major
    solvers: Optional[list] = None
    uexact: Optional[Callable] = None
    info: dict = field(default_factory=dict)


def build_schur_problem(N: int, px: int, py: int, coeff: Coeff, f, uexact,
                        assemble: bool = True, precond: bool = True, dom_slice=None,
                        mesh: Optional[Mesh] = None, partition=None, blocks=None, sub: Optional[Subdomains] = None,
                        dense_setup=None) -> SchurProblem:
    """Example03:45-150 set-up flow on the synthetic mesh (mesh → partition → maps →
    local blocks → b_schur → assembled S_d → Neumann-Neumann pseudo-inverses).

    `dom_slice=(lo, hi)` (multi-GPU: one call per rank) factorises, assembles and pseudo-inverts
    only subdomains lo..hi-1; the other entries of `solvers`, `Sd`, `ΠSd` are None and
    `b_schur` then holds only this rank's share  -Σ_{d in slice} R_d' A_IΓd' A_IId^{-1} b_Id
    (+ b_Γ on the rank that owns subdomain 0), so that the sum over ranks is the full b_schur.
    `mesh` / `partition=(epart, npart)` replace the structured substitutes, e.g. with files written by the
    reference's Triangle + METIS pipeline (io.load_mesh / io.load_partition).
    `blocks=(A_IIdd, A_IΓdd, A_ΓΓdd, b_Id, b_Γ)` skips the element loop (e.g. `AssemblyPlan.blocks` of values
    assembled on the GPU; `coeff` is then unused) and `sub` re-uses the subdomain maps of an earlier call.
    """
    mesh = get_mesh(N) if mesh is None else mesh
    dinds = get_dirichlet_inds(mesh.points, mesh.point_marker)
    epart, npart = mesh_partition(mesh, px, py) if partition is None else partition
    if sub is None:
        sub = set_subdomains(mesh.cells, mesh.cell_neighbors, epart, npart, dinds.dirichlet_g2l)
    if blocks is None:
        blocks = prepare_local_schurs(mesh.cells, mesh.points, epart, sub, coeff, f, uexact)
    A_II, A_IΓ, A_ΓΓ, b_Id, b_Γ = blocks
    lo, hi = (0, sub.ndom) if dom_slice is None else dom_slice
    loc = range(lo, hi)
    b_schur = np.array(b_Γ, copy=True) if lo == 0 else np.zeros_like(b_Γ)
    solvers = LazySolvers(A_II, lo, hi)          # SuperLU factors, built only if something asks for them
    Sd = Pi = None
    if assemble:
        # one elimination per subdomain gives S_d and the condensed rhs (get_schur_rhs, EPDD.jl:835-864)
        # `dense_setup(A_II, A_IΓ, A_ΓΓ, b_Id, want_pinv) -> (S_d list, w_d list, ΠS_d list | None)`: e.g. the device set-up of the
        # library (api.device_dense_setup: mi_schur_setup_run + mi_nn_pinv) in place of this module's host elimination
        Pl = None
        if dense_setup is not None:
            Sl, wl, Pl = dense_setup([A_II[d] for d in loc], [A_IΓ[d] for d in loc], [A_ΓΓ[d] for d in loc],
                                     [b_Id[d] for d in loc], precond)
        else:
            Sl, wl = assemble_local_schurs([A_II[d] for d in loc], [A_IΓ[d] for d in loc], [A_ΓΓ[d] for d in loc],
                                           b_Id=[b_Id[d] for d in loc])
        for d in loc:
            b_schur[sub.gather_idx[d]] -= wl[d - lo]
        Sd = [Sl[d - lo] if lo <= d < hi else None for d in range(sub.ndom)]
        if precond:
            if Pl is None:
                Pl = prepare_neumann_neumann_schur_precond(Sl)
            Pi = [Pl[d - lo] if lo <= d < hi else None for d in range(sub.ndom)]
    else:
        for d in loc:                           # get_schur_rhs with sparse direct interior solves
            b_schur[sub.gather_idx[d]] -= A_IΓ[d].T @ solvers[d](b_Id[d])
    prob = SchurProblem(mesh, dinds, sub, epart, A_II, A_IΓ, A_ΓΓ, b_Id, b_Γ, b_schur,
                        solvers=solvers, uexact=uexact)
    prob.info["dom_slice"] = (lo, hi)
    prob.Sd, prob.ΠSd = Sd, Pi
    return prob


# --------------------------------------------------------------------------------------
# Quantization of ξ (Examples 12-14, 18, 20), host side, in the orders of the device kernels (csrc/vq.hpp): the results
# below carry the bits of api.vq_assign / kmeans / ... . X is d x ns (a sample per column), C is d x P (a centroid per
# column), indices are 0-based. "Ex12F" = Example12_Quantization_Functions.jl, "Ex13F" = Example13_CLVQ_Functions.jl,
# "Ex14F" = Example14_QuantizationAndShepardLocalInterpolation_Functions.jl, "Ex20F" =
# Example20_QuantizedPreconditioner_Functions.jl.
# --------------------------------------------------------------------------------------
VQ_SUM_CHUNK = 256          # samples per chunk of the ordered sums (mi_vq_tiling's sum_chunk)


def vq_dist2(X, C):
    """dist2[s, p] = (x_s .- c_p)' * (x_s .- c_p) as a loop: t = x_k - c_k, acc = acc + t * t, k ascending from +0."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    acc = np.zeros((X.shape[1], C.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(X.shape[0]):
            t = X[k, :, None] - C[k, None, :]
            acc = acc + t * t
    return acc


def vq_scan(D):
    """The reference's strict `<` scan over the columns of D (ns x P), started at column 0 (Ex20F:44-52): a NaN in column 0
    stays, a NaN elsewhere never wins, among equals the lowest p wins."""
    best, arg = D[:, 0].copy(), np.zeros(D.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(1, D.shape[1]):
            m = D[:, p] < best
            best[m], arg[m] = D[m, p], p
    return arg, best


def vq_assign(X, C, block: int = 2048):
    """Nearest centroid and its squared distance for every column of X -> (assign, dist2)."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    ns = X.shape[1]
    a, c = np.zeros(ns, dtype=np.int64), np.zeros(ns)
    for s0 in range(0, ns, block):
        a[s0:s0 + block], c[s0:s0 + block] = vq_scan(vq_dist2(X[:, s0:s0 + block], C))
    return a, c


def vq_chunk_sums(v, chunk: int = VQ_SUM_CHUNK):
    """The ordered sums over samples: (excl, within, total). within[s] = ascending sum inside the chunk of s up to and
    including s; excl[c] = ascending sum of the totals of the chunks before c; total = excl[-1] + (last chunk's total)."""
    v = np.asarray(v, dtype=np.float64)
    nch = (v.size + chunk - 1) // chunk
    within, tot = np.empty(v.size), np.empty(nch)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(nch):
            w = np.cumsum(v[c * chunk:(c + 1) * chunk])      # sequential: ((v0 + v1) + v2) + ...
            within[c * chunk:c * chunk + w.size], tot[c] = w, w[-1]
        excl = np.concatenate(([0.0], np.cumsum(tot)[:-1]))
        total = excl[-1] + tot[-1]
    return excl, within, float(total)


def vq_objective(dist2, chunk: int = VQ_SUM_CHUNK) -> float:
    """objv = Σ_s dist2[s] in the chunked order."""
    return vq_chunk_sums(dist2, chunk)[2]


def get_distortion(X, hXt) -> float:
    """`get_distortion` (Ex13F:53-69): w2 = (Σ_s min_p dist2) / ns, the sum in the chunked order."""
    return vq_objective(vq_assign(X, hXt)[1]) / np.asarray(X).shape[1]


def vq_update(X, assign, C):
    """Lloyd's centre update -> (C_new, counts): sum[:, a[s]] += X[:, s] for s ascending from +0, then a true division by the
    count; a cluster without a member keeps its centre bit for bit (Clustering.jl would repick it at random)."""
    X, C = np.asarray(X, dtype=np.float64), np.array(C, dtype=np.float64)
    assign = np.asarray(assign, dtype=np.int64)
    P = C.shape[1]
    if assign.size and (assign.min() < 0 or assign.max() >= P):
        raise ValueError("assignment outside [0, P)")
    sums = np.zeros((P, X.shape[0]))
    np.add.at(sums, assign, X.T)                             # unbuffered: one sample after the other, s ascending
    counts = np.bincount(assign, minlength=P).astype(np.int64)
    live = counts > 0
    C[:, live] = (sums[live] / counts[live, None]).T
    return C, counts


def kmpp_seed(X, P: int, u, chunk: int = VQ_SUM_CHUNK):
    """k-means++ on P uniforms u[j] in [0, 1) -> (picked, C). Centre 0 is sample floor(u[0] ns); then mind = min(mind,
    dist2(·, c_{j-1})), prefix(s) = excl[chunk of s] + within[s], and the pick is the smallest s with prefix(s) > u[j] total
    (where rounding leaves none: the smallest s with prefix(s) >= total). total == 0 raises ValueError."""
    X, u = np.asarray(X, dtype=np.float64), np.asarray(u, dtype=np.float64)
    d, ns = X.shape
    if P > ns or u.size < P:
        raise ValueError("P > ns, or fewer than P uniforms")
    picked = np.zeros(P, dtype=np.int64)
    f = np.floor(u[0] * float(ns))
    picked[0] = int(min(f, ns - 1)) if f >= 0 else 0
    mind = np.full(ns, np.inf)
    for j in range(1, P):
        dj = vq_dist2(X, X[:, picked[j - 1]][:, None])[:, 0]
        mind = np.where(dj < mind, dj, mind)
        excl, within, total = vq_chunk_sums(mind, chunk)
        if not (total > 0.0) or not np.isfinite(total):
            raise ValueError("the distances to the centres chosen so far sum to 0: fewer distinct points than centres")
        prefix = np.repeat(excl, chunk)[:ns] + within
        hit = np.nonzero(prefix > u[j] * total)[0]
        if hit.size == 0:
            hit = np.nonzero(prefix >= total)[0]
        picked[j] = hit[0]
    return picked, X[:, picked].copy()


@dataclass
class KmeansResult:
    """The fields of Clustering.jl's KmeansResult the reference reads (0-based assignments)."""
    centers: np.ndarray
    assignments: np.ndarray
    costs: np.ndarray
    counts: np.ndarray
    totalcost: float
    iterations: int
    converged: bool


def kmeans(X, C0, tol: float = 1e-8, maxiter: int = 1000) -> KmeansResult:
    """Lloyd's algorithm from the centres C0, the loop of mi_vq_kmeans: assign; then update, assign, and stop when the
    objective changed by less than `tol` in absolute value (Clustering.jl's documented rule, restated) or after maxiter."""
    X, C = np.asarray(X, dtype=np.float64), np.array(C0, dtype=np.float64)
    a, c = vq_assign(X, C)
    objv = vq_objective(c)
    if not np.isfinite(objv):
        raise ValueError("the objective after the first assignment is not finite")
    counts = np.zeros(C.shape[1], dtype=np.int64)
    t, converged = 0, False
    while not converged and t < maxiter:
        t += 1
        C, counts = vq_update(X, a, C)
        a, c = vq_assign(X, C)
        prev, objv = objv, vq_objective(c)
        converged = bool(abs(objv - prev) < tol)
    return KmeansResult(C, a, c, counts, objv, t, converged)


def find_precond(x, hXt) -> int:
    """`find_precond` (Ex20F:39-54): the centroids are zero-padded from nKL_trunc to length(x); 0-based index."""
    x, hXt = np.asarray(x, dtype=np.float64), np.asarray(hXt, dtype=np.float64)
    padded = np.zeros((x.size, hXt.shape[1]))
    padded[:hXt.shape[0]] = hXt
    return int(vq_assign(x[:, None], padded)[0][0])


def _vq_rows(Λ, distance: str) -> int:
    """Rows the quantizer of this distance works on: all of them, or, for "L2-10%", up to the first α with
    cumsum(Λ)[α] >= 0.1 (Ex12F:45)."""
    Λ = np.asarray(Λ, dtype=np.float64)
    if distance != "L2-10%":
        return Λ.size
    hit = np.nonzero(np.cumsum(Λ) >= 0.1)[0]
    if hit.size == 0:
        raise ValueError('"L2-10%": cumsum(Λ) never reaches 0.1 (the reference\'s findfirst returns nothing)')
    return int(hit[0]) + 1


def scale_data(ξ, Λ, distance: str):
    """`scale_data` (Ex20F:24-37) for one vector or for the columns of a matrix; a copy is returned. Distances: "L2" /
    "L2-full" (ξ .* sqrt(Λ)), "cdf" (cdf.(Normal(), ξ) .* sqrt(Λ), Ex20F:16-18), "cdf-full" (cdf only, Ex12F:52) and "L2-10%"
    (the rows of _vq_rows, scaled as "L2": Ex12F:44-47)."""
    from scipy.special import ndtr
    Λ = np.asarray(Λ, dtype=np.float64)
    Y = np.array(ξ, dtype=np.float64)
    sq = np.sqrt(Λ) if Y.ndim == 1 else np.sqrt(Λ)[:, None]
    if distance in ("L2", "L2-full"):
        return Y * sq
    if distance == "cdf":
        return ndtr(Y) * sq
    if distance == "cdf-full":
        return ndtr(Y)
    if distance == "L2-10%":
        r = _vq_rows(Λ, distance)
        return Y[:r] * sq[:r]
    raise ValueError(f"unknown distance {distance!r}")


def unscale_centers(C, Λ, distance: str):
    """Centres of the scaled data back to ξ (Ex20F:66-71, Ex12F:42, 49, 55): the inverse of scale_data on its rows."""
    from scipy.special import ndtri
    C = np.array(C, dtype=np.float64)
    sq = np.sqrt(np.asarray(Λ, dtype=np.float64)[:C.shape[0]])[:, None]
    if distance in ("L2", "L2-full", "L2-10%"):
        return C / sq
    if distance == "cdf":
        return ndtri(C / sq)
    if distance == "cdf-full":
        return ndtri(C)
    raise ValueError(f"unknown distance {distance!r}")


def get_scaled_data(ns: int, Λ, distance: str, rng: np.random.Generator):
    """`get_scaled_data` (Ex20F:5-22): ns draws of ξ ~ N(0, I) as columns, scaled for `distance`. The reference seeds Julia's
    generator with 987_654_321; here the caller brings the generator."""
    return scale_data(rng.standard_normal((np.asarray(Λ).size, ns)), Λ, distance)


def get_deterministic_grid(P: int, nKL: int, Λ, s: float):
    """`get_deterministic_grid` (Ex20F:75-93) -> (hηt, hξt), nKL x P: column 0 is ξ = 0, column p = 1 .. 2^nKL holds -s / +s by
    the last nKL bits of p (most significant first; p = 2^nKL gives all -s). The reference leaves further columns undefined;
    here they are zero."""
    if P < (1 << nKL) + 1 and nKL > 0:
        raise ValueError(f"P = {P} columns cannot hold 0 and the 2^{nKL} corners")
    hξt = np.zeros((nKL, P))
    if nKL > 0:
        for p in range(1, (1 << nKL) + 1):
            for k in range(nKL):
                hξt[k, p] = s if (p >> (nKL - 1 - k)) & 1 else -s
    return np.sqrt(np.asarray(Λ, dtype=np.float64)[:nKL])[:, None] * hξt, hξt


def get_gain_sequence(γ0: float, α: float, β: float, c: float, ns: int):
    """`get_gain_sequence` (Ex13F:45-51): γ[t] = γ0 α / (t^c + β), t = 1 .. ns."""
    t = np.arange(1, ns + 1, dtype=np.float64)
    return γ0 * α / (t ** c + β)


def clvq(X, P: int, γ, init):
    """`clvq` (Ex13F:71-92): competitive learning, one sample after the other — sequential by construction, so it stays on the
    host. `init`: P sample indices (the reference's initialize_quantizer draws them at random, Ex13F:23-43) or a d x P
    codebook. The competitive phase is the strict `<` scan on the loop form of the distance."""
    X = np.asarray(X, dtype=np.float64)
    init = np.asarray(init)
    H = X[:, init.astype(np.int64)].copy() if init.ndim == 1 else np.array(init, dtype=np.float64)
    if H.shape != (X.shape[0], P):
        raise ValueError("init: P sample indices or a d x P codebook")
    for t in range(X.shape[1]):
        a, _ = vq_scan(vq_dist2(X[:, t:t + 1], H))
        p = int(a[0])
        H[:, p] -= γ[t] * (H[:, p] - X[:, t])
    return H


def shepard_coefficients(ξ, interpolators, Λ, distance: str = "L2-full"):
    """The coefficients of `shepard_interpolating_precond` (Ex14F:174-206), exactly as written there: Δξ = (interpolators[:, i]
    .- ξ) .* Λ — weighted with Λ, not sqrt.(Λ): the reference's quirk, kept — d_i = sqrt(Δξ'Δξ), W = Σ 1 / d_i²,
    c_i = (1 / d_i²) / W. A zero distance gives non-finite coefficients, as it does there."""
    from scipy.special import ndtr
    ξ, I, Λ = np.asarray(ξ, dtype=np.float64), np.asarray(interpolators, dtype=np.float64), np.asarray(Λ, dtype=np.float64)
    n = I.shape[1]
    dist = np.empty(n)
    W = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            if distance == "L2-full":
                Δ = (I[:, i] - ξ) * Λ
            elif distance == "cdf-full":
                Δ = ndtr(I[:, i] - ξ)
            else:
                raise ValueError(f"unknown distance {distance!r}")
            dist[i] = np.sqrt(np.dot(Δ, Δ))
            W += 1.0 / dist[i] ** 2
        return (1.0 / dist ** 2) / W
