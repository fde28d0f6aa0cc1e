"""The quantizer of Examples 12-14, 18, 20 in loop form, on the host: what csrc/vq.hpp and fem.py's quantizer functions are
held to, bit for bit. Written on its own (it imports nothing of the package).

Not a conftest: tests/test_vq_cpu.py and tests/test_gpu_vq.py import it.

Orders. dist2(x, c): t = x[k] - c[k], acc = acc + t * t, k ascending from +0 — `(x .- c)' * (x .- c)` as a loop
(Example20_QuantizedPreconditioner_Functions.jl:44-47); a loop over p and k on vectors of samples, whose elementwise numpy
operations round like the scalars. The scan is the reference's strict `<`, started at centroid 0. Sums over samples: chunks
of `chunk` consecutive samples added in ascending order (np.cumsum is sequential), then the chunk totals in ascending order.
"""
import numpy as np


def dist2(X, C):
    """(ns, P)"""
    d, ns = X.shape
    P = C.shape[1]
    D = np.empty((ns, P))
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            acc = np.zeros(ns)
            for k in range(d):
                t = X[k, :] - C[k, p]
                acc = acc + t * t
            D[:, p] = acc
    return D


def assign(X, C):
    """(assign, dist2): min_dist = dist(c_0); for p >= 1: if dist < min_dist: take it"""
    D = dist2(X, C)
    best, arg = D[:, 0].copy(), np.zeros(D.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(1, D.shape[1]):
            for s in np.nonzero(D[:, p] < best)[0]:
                best[s], arg[s] = D[s, p], p
    return arg, best


def chunked(v, chunk):
    """(prefix, total): prefix[s] = (ascending sum of the totals of the earlier chunks) + (ascending sum within the chunk of s
    up to and including s); total = prefix[-1]"""
    v = np.asarray(v, dtype=np.float64)
    prefix = np.empty(v.size)
    earlier = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, v.size, chunk):
            w = np.cumsum(v[b:b + chunk])
            prefix[b:b + chunk] = earlier + w
            earlier = earlier + w[-1]
    return prefix, float(prefix[-1])


def objective(v, chunk):
    return chunked(v, chunk)[1]


def update(X, a, C):
    """(C_new, counts): for s: sum[:, a[s]] += X[:, s]; C[:, p] = sum[:, p] / count[p]; an empty cluster keeps its centre"""
    d, ns = X.shape
    P = C.shape[1]
    sums, counts = np.zeros((d, P)), np.zeros(P, dtype=np.int64)
    for s in range(ns):
        sums[:, a[s]] = sums[:, a[s]] + X[:, s]
        counts[a[s]] += 1
    out = C.copy()
    for p in range(P):
        if counts[p] > 0:
            out[:, p] = sums[:, p] / float(counts[p])
    return out, counts


def seed(X, P, u, chunk):
    """k-means++ on the uniforms u -> (picked, C), or None when the distances to the chosen centres sum to 0"""
    d, ns = X.shape
    picked = np.zeros(P, dtype=np.int64)
    picked[0] = min(int(np.floor(u[0] * float(ns))), ns - 1)
    mind = np.full(ns, np.inf)
    for j in range(1, P):
        dj = dist2(X, X[:, picked[j - 1]:picked[j - 1] + 1])[:, 0]
        for s in range(ns):
            if dj[s] < mind[s]:
                mind[s] = dj[s]
        prefix, total = chunked(mind, chunk)
        if total == 0.0:
            return None
        thresh = u[j] * total
        hit = [s for s in range(ns) if prefix[s] > thresh]
        if not hit:
            hit = [s for s in range(ns) if prefix[s] >= total]
        picked[j] = hit[0]
    return picked, X[:, picked].copy()


def kmeans(X, C0, chunk, tol=1e-8, maxiter=1000):
    """dict(centers, assignments, costs, counts, totalcost, iterations, converged, changes): the loop of mi_vq_kmeans"""
    C = C0.copy()
    a, c = assign(X, C)
    objv = objective(c, chunk)
    counts = np.zeros(C.shape[1], dtype=np.int64)
    t, converged, changes = 0, False, []
    while not converged and t < maxiter:
        t += 1
        C, counts = update(X, a, C)
        a, c = assign(X, C)
        prev, objv = objv, objective(c, chunk)
        changes.append(abs(objv - prev))
        converged = abs(objv - prev) < tol
    return dict(centers=C, assignments=a, costs=c, counts=counts, totalcost=objv, iterations=t, converged=converged, changes=changes)


def find_precond(x, hXt):
    """Example20_…_Functions.jl:39-54, 0-based"""
    padded = np.zeros((x.size, hXt.shape[1]))
    padded[:hXt.shape[0], :] = hXt
    return int(assign(x.reshape(-1, 1), padded)[0][0])


def clvq(X, H0, gamma):
    """Example13_CLVQ_Functions.jl:71-92 from the codebook H0, scalar loops"""
    d, ns = X.shape
    H = H0.copy()
    P = H.shape[1]
    for t in range(ns):
        best, pmin = None, 0
        for p in range(P):
            acc = 0.0
            for k in range(d):
                df = X[k, t] - H[k, p]
                acc = acc + df * df
            if p == 0 or acc < best:
                best, pmin = acc, p
        for k in range(d):
            H[k, pmin] = H[k, pmin] - gamma[t] * (H[k, pmin] - X[k, t])
    return H
