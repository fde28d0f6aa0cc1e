"""numpy restatement of the reference's Karhunen-Loève layer (Fem/KarhunenLoeve.jl, Fem/KarhunenLoeveDomainDecomposition.jl =
"KLDD.jl", Fem/Covariances.jl) for tests/test_kl_cpu.py and tests/test_gpu_kl.py: dense K, M and C = M K M, the literal element
loops, `eigh(C, M)`, the keep loops, the reduced assembly block by block, project_on_mesh, and the derived error bound of the
covariance kernel. Everything is dense and 0-based; nothing here imports the package under test except where a function takes
`fem` as an argument (the mesh)."""
import functools

import numpy as np
import scipy.linalg as sla

EPS = 2.0 ** -52
T_CAP = 745.0          # exp(-t) is 0 in fp64 beyond t = 745.13...


# ------------------------------------------------------------------ covariance
def exponent(model, sig2, L, pt, ps):
    """t[i, j] >= 0, the magnitude of the exponent of cov(pt[:, i], ps[:, j]), as the reference writes it (Covariances.jl:27)."""
    dx = pt[0][:, None] - ps[0][None, :]
    dy = pt[1][:, None] - ps[1][None, :]
    r2 = dx ** 2 + dy ** 2
    if model == "SExp":
        return r2 / L ** 2
    if model == "Exp":
        return np.sqrt(r2) / L
    raise ValueError(model)


def dense_K(model, sig2, L, pt, ps):
    return sig2 * np.exp(-exponent(model, sig2, L, pt, ps))


def cov_scalar(model, sig2, L):
    """cov(x1, y1, x2, y2) on scalars, the callable the reference passes around (Example02:30-34)."""
    def cov(x1, y1, x2, y2):
        if model == "SExp":
            return sig2 * np.exp(-((x1 - x2) ** 2 + (y1 - y2) ** 2) / L ** 2)
        return sig2 * np.exp(-np.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2) / L)
    return cov


def kernel_bound(model, sig2, L, pt, ps, X):
    """Derived bound on |Y - Y_ref|, per entry, for Y = K X computed in any summation order with one exp per pair:
        2 eps Σ_j (ns + 4 min(t_ij, 745) + 16) K_ij |X_j|
    ns: the summation; 4 t: the rounding of the exponent (differences, squares, sum, division: 4 roundings of relative size
    eps, amplified by exp to t eps each); 16: exp's own ulp, the product with sig2 and with X, with slack; the leading 2: the
    restatement's own rounding."""
    X = np.asarray(X, dtype=np.float64).reshape(ps.shape[1], -1)
    t = exponent(model, sig2, L, pt, ps)
    w = (ps.shape[1] + 4.0 * np.minimum(t, T_CAP) + 16.0) * (sig2 * np.exp(-t))
    return 2.0 * EPS * (w @ np.abs(X))


# ------------------------------------------------------------------ mass matrices and C
def areas(cells, points):
    x, y = points[0][cells], points[1][cells]
    dx = np.stack([x[2] - x[1], x[0] - x[2], x[1] - x[0]])
    dy = np.stack([y[1] - y[2], y[2] - y[0], y[0] - y[1]])
    return (dx[2] * dy[1] - dx[1] * dy[2]) / 2.0


def dense_mass(cells, points, nodes=None, elems=None):
    """get_mass_matrix (EllipticPde.jl:412-466) / do_local_mass_assembly (KLDD.jl:236-293), dense, in the numbering `nodes`."""
    nnode = points.shape[1]
    nodes = np.arange(nnode) if nodes is None else np.asarray(nodes)
    elems = np.arange(cells.shape[1]) if elems is None else np.asarray(elems)
    g2l = np.full(nnode, -1)
    g2l[nodes] = np.arange(nodes.size)
    A = areas(cells, points)
    M = np.zeros((nodes.size, nodes.size))
    for el in elems:
        for i in range(3):
            for j in range(3):
                M[g2l[cells[i, el]], g2l[cells[j, el]]] += A[el] / 6.0 if i == j else A[el] / 12.0
    return M


def loops_C(cells, points, cov, nodes_i, elems_i, nodes_j, elems_j):
    """The two element loops of the reference, literally (KarhunenLoeve.jl:40-105; rectangular form KLDD.jl:505-586):
    R[i, j] += (2 cov(p_r, p_j) + cov(p_s, p_j) + cov(p_t, p_j)) Area / 12 over the elements of the ROW set, then
    C[i, j] += (2 R[i, j] + R[i, k] + R[i, ℓ]) Area / 12 over the elements of the COLUMN set."""
    nnode = points.shape[1]
    gi = np.full(nnode, -1); gi[nodes_i] = np.arange(len(nodes_i))
    gj = np.full(nnode, -1); gj[nodes_j] = np.arange(len(nodes_j))
    A = areas(cells, points)
    R = np.zeros((len(nodes_i), len(nodes_j)))
    C = np.zeros((len(nodes_i), len(nodes_j)))
    for j, jnode in enumerate(nodes_j):
        xj, yj = points[0, jnode], points[1, jnode]
        for el in elems_i:
            x, y = points[0, cells[:, el]], points[1, cells[:, el]]
            for r in range(3):
                s, t = (r + 1) % 3, (r + 2) % 3
                R[gi[cells[r, el]], j] += (2 * cov(x[r], y[r], xj, yj) + cov(x[s], y[s], xj, yj) + cov(x[t], y[t], xj, yj)) * A[el] / 12
    for el in elems_j:
        for r in range(3):
            s, t = (r + 1) % 3, (r + 2) % 3
            j, k, l = gj[cells[r, el]], gj[cells[s, el]], gj[cells[t, el]]
            C[:, j] += (2 * R[:, j] + R[:, k] + R[:, l]) * A[el] / 12
    return C


def set_subdomain(cells, points, epart, idom):
    """KLDD.jl:40-80: nodes in first-seen order, the elements, the mean of the nodes."""
    l2g, seen, elems = [], set(), []
    for el in range(cells.shape[1]):
        if epart[el] == idom:
            elems.append(el)
            for node in cells[:, el]:
                if int(node) not in seen:
                    seen.add(int(node))
                    l2g.append(int(node))
    l2g = np.array(l2g)
    return l2g, np.array(elems), points[:, l2g].sum(axis=1) / l2g.size


# ------------------------------------------------------------------ eigenproblems and keep loops
def eigh_desc(C, M):
    """scipy.linalg.eigh(C, M), most dominant first; V' M V = I."""
    lam, V = sla.eigh((C + C.T) / 2, M)
    return lam[::-1].copy(), V[:, ::-1].copy()


def energy(cells, points, elems=None):
    """(Area, centre) of KarhunenLoeve.jl:145-165 (centre: mean of the element centroids)."""
    elems = np.arange(cells.shape[1]) if elems is None else elems
    A = areas(cells, points)[elems]
    cen = points[:, cells[:, elems]].mean(axis=1).mean(axis=1)
    return float(A.sum()), cen


def keep(lam, energy_expected):
    """KarhunenLoeve.jl:169-180 -> nvec, cumulative energies"""
    acc, nvec, cum = 0.0, 0, []
    for v in lam:
        if v > 0:
            nvec += 1
            acc += v
            cum.append(acc)
        else:
            break
        if acc >= energy_expected:
            break
    return nvec, cum


def reduced_block(model, sig2, L, points, nodes_i, M_i, Phi_i, nodes_j, M_j, Phi_j):
    """Block (idom, jdom) of KLDD.jl:588-606: Φ_i' C_ij Φ_j with C_ij = M_i K(P_i, P_j) M_j dense."""
    Kd = dense_K(model, sig2, L, points[:, nodes_i], points[:, nodes_j])
    return Phi_i.T @ (M_i @ Kd @ M_j) @ Phi_j


def project_on_mesh(nnodes, Phi, inds_l2gd, Phid):
    """KLDD.jl:920-959, literally."""
    nmodes = Phi.shape[1]
    Psi = np.zeros((nnodes, nmodes))
    md = [P.shape[1] for P in Phid]
    for imode in range(nmodes):
        cnt = np.zeros(nnodes, dtype=int)
        for idom, l2g in enumerate(inds_l2gd):
            for i, inode in enumerate(l2g):
                cnt[inode] += 1
                for a in range(md[idom]):
                    Psi[inode, imode] += Phi[sum(md[:idom]) + a, imode] * Phid[idom][i, a]
        Psi[:, imode] /= cnt
    return Psi


def draw(Lam, Psi, xi):
    """KLDD.jl:985-999 with a given ξ."""
    g = np.zeros(Psi.shape[0])
    for a in range(Lam.size):
        g += np.sqrt(Lam[a]) * xi[a] * Psi[:, a]
    return g


# ------------------------------------------------------------------ the shared 400-node problem (computed once)
N_SIDE, L_GLOBAL, SIG2 = 20, 0.3, 1.0


@functools.lru_cache(maxsize=None)
def problem400(fem):
    """get_mesh(20): 400 nodes, L = 0.3, σ² = 1 — (mesh, M, K, C, λ, V) with (λ, V) = eigh(C, M) descending."""
    mesh = fem.get_mesh(N_SIDE)
    M = dense_mass(mesh.cells, mesh.points)
    K = dense_K("SExp", SIG2, L_GLOBAL, mesh.points, mesh.points)
    C = M @ K @ M
    lam, V = eigh_desc(C, M)
    for a in (M, K, C, lam, V):
        a.setflags(write=False)
    return mesh, M, K, C, lam, V
