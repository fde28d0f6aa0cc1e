"""Host-side mirror of the reference's operator / preconditioner / solver interface for the
Schur-PCG hot path, on top of the C ABI (include/mi355schur.h). Same names, argument order and
return values as the Julia functions; citations are relative to /root/reference
("EPDD.jl" = Fem/EllipticPdeDomainDecomposition.jl).

    cg(A, b, x; maxit=0)            -> (x, it, res_norm[1:it])     RecyclingKrylovSolvers/cg.jl:14
    pcg(A, b, x, M; maxit=0)                                        cg.jl:67
    defcg(A, b, x, W; maxit=0)                                      defcg.jl:24
    defpcg(A, b, x, W, M; maxit=0)                                  defcg.jl:242
    apply_local_schurs(S, x)  /  S * x                              EPDD.jl:711-785
    apply_global_schur(S, x)                                        EPDD.jl:596-625
    NeumannNeumannSchurPreconditioner(ΠSd, ind_Γd_Γ2l, node_Γ_cnt)  EPDD.jl:1111-1137
    apply_neumann_neumann_schur(Πnn, r)  /  Πnn.ldiv(r)             EPDD.jl:1361-1403

Vectors may be numpy arrays (host pointers; copied through the boundary like Julia arrays) or
torch CUDA tensors (device pointers, zero copy). Indices are 0-based (`index_base=0`); a Julia
caller passes `index_base=1` through the shim in julia/MI355Schur.jl.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import (BoundsError, MiError, SingularException, check, f64p, f64pp, i64, i64p, i64pp, vp)  # noqa: F401

EPS = 1e-7  # RecyclingKrylovSolvers.jl:21 `const eps = 1e-7`


def _is_torch(x) -> bool:
    t = type(x)
    return t is not np.ndarray and t.__module__.startswith("torch")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptrs(arrs, elem_ptr_type):
    """C array of pointers; None entries become NULL (other ranks' subdomains)."""
    out = (elem_ptr_type * len(arrs))()
    for k, a in enumerate(arrs):
        out[k] = a.ctypes.data_as(elem_ptr_type) if a is not None else None
    return out


class Context:
    """One GPU + one HIP stream (+ an optional RCCL communicator). `mi_ctx_t`."""

    def __init__(self, device: int = 0):
        L = _lib.load()
        h = vp()
        check(L.mi_ctx_create(C.c_int(device), C.byref(h)))
        self._h, self._L, self.device = h, L, device
        self.rank, self.n_ranks = 0, 1

    # -- pointer mode follows the argument type of each call
    def _mode_for(self, *vecs) -> int:
        dev = [v for v in vecs if v is not None and _is_torch(v)]
        if dev and len(dev) != len([v for v in vecs if v is not None]):
            raise TypeError("mix of torch tensors and numpy arrays in one call")
        mode = _lib.MI_PTR_DEVICE if dev else _lib.MI_PTR_HOST
        check(self._L.mi_ctx_set_pointer_mode(self._h, mode))
        return mode

    def _res_buffer(self, cap: int):
        """Landing zone of a solve's residual history, kept per context (one allocation and one address lookup instead of
        one per solve: `ndarray.ctypes` alone costs several microseconds, a fifth of what a 15-iteration solve's launch does)."""
        buf = getattr(self, "_res", None)
        if buf is None or buf[0].size < cap:
            a = np.empty(max(cap, 64))
            buf = self._res = (a, C.cast(a.ctypes.data, f64p))
        return buf

    @staticmethod
    def _ptr(v, n: Optional[int] = None, writable: bool = False):
        """(keepalive, void*) of a contiguous fp64 vector."""
        if v is None:
            return None, None
        if _is_torch(v):
            import torch
            if v.dtype != torch.float64 or not v.is_cuda or not v.is_contiguous():
                raise TypeError("device vectors must be contiguous float64 CUDA tensors")
            if n is not None and v.numel() != n:
                raise ValueError(f"expected {n} entries, got {v.numel()}")
            return v, vp(v.data_ptr())
        a = v if (isinstance(v, np.ndarray) and v.dtype == np.float64 and v.flags.c_contiguous
                  and (v.flags.writeable or not writable)) else _f64(v)
        if n is not None and a.size != n:
            raise ValueError(f"expected {n} entries, got {a.size}")
        return a, vp(a.ctypes.data)

    def loopback_init(self, group: "LoopbackGroup", rank: int) -> None:
        """Make this context rank `rank` of an in-process group (one host thread per rank): the single-GPU stand-in for
        `comm_init`, used to test the sharded operators (`mi_ctx_loopback_init`)."""
        check(self._L.mi_ctx_loopback_init(self._h, group._h, C.c_int(rank)))
        self.rank, self.n_ranks, self._group = rank, group.n, group

    def set_chunk(self, iterations_per_graph: int) -> None:
        check(self._L.mi_ctx_set_chunk(self._h, C.c_int(iterations_per_graph)))

    def use_torch_stream(self) -> None:
        """Launch on torch's current stream (so torch.cuda.Event sees our kernels, and tensors produced by torch kernels
        just before a call are ordered with it). Not the legacy default stream: the solvers capture graphs."""
        import torch
        check(self._L.mi_ctx_set_stream(self._h, vp(torch.cuda.current_stream(self.device).cuda_stream)))

    def use_own_stream(self) -> None:
        check(self._L.mi_ctx_set_stream(self._h, None))

    def _record(self, *tensors) -> None:
        """Asynchronous entry points (`mi_dense_set_blocks`, `mi_schur_setup_run`, `mi_nn_pinv`, `mi_assembly_run` in
        device-pointer mode) return while the context's stream still reads / writes the caller's torch tensors. Torch's
        current stream is made to wait for the context's stream at this point (an event, no host synchronisation), so a
        tensor that dies right after the call is not handed out again — on torch's stream — before the work is done.
        (Not `Tensor.record_stream`: the allocator would record an event on the context's stream when the tensor is freed,
        possibly after the context — and its stream — are gone.) Contract: INTEGRATION.md "device pointers"."""
        self._order(tensors, after=True)

    def _order(self, tensors, after: bool) -> None:
        """The Python operators that hand torch tensors back (`A * x`, `schur_rhs`, `interior_solutions`) behave like torch
        ops: the context's stream waits for torch's current stream before the call, torch's current stream waits for the
        context's after it (two events, no host synchronisation), and the allocator is told (`_record`). The bare C entry
        points keep the contract of INTEGRATION.md: ordering is the caller's."""
        ts = [t for t in tensors if t is not None and _is_torch(t) and t.is_cuda]
        if not ts:
            return
        import torch
        sp = vp()
        check(self._L.mi_ctx_get_stream(self._h, C.byref(sp)))
        cur = torch.cuda.current_stream(ts[0].device)
        if not sp.value or cur.cuda_stream == sp.value:
            return
        ext = torch.cuda.ExternalStream(sp.value, device=ts[0].device)
        if after:
            cur.wait_stream(ext)
        else:
            ext.wait_stream(cur)

    def synchronize(self) -> None:
        check(self._L.mi_ctx_synchronize(self._h))

    # -- RCCL
    def unique_id(self) -> bytes:
        buf = C.create_string_buffer(_lib.MI_COMM_ID_BYTES)
        check(self._L.mi_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, n_ranks: int) -> None:
        buf = C.create_string_buffer(uid, _lib.MI_COMM_ID_BYTES)
        check(self._L.mi_ctx_comm_init(self._h, buf, C.c_int(rank), C.c_int(n_ranks)))
        self.rank, self.n_ranks = rank, n_ranks

    # -- the one-shot peer exchange (include/mi355schur.h; `@distributed (+)`, EllipticPdePllDomainDecomposition.jl:10-14)
    def peer_init(self, rank: int, n_ranks: int, arena_bytes: int = 0) -> None:
        check(self._L.mi_ctx_peer_init(self._h, C.c_int(rank), C.c_int(n_ranks), i64(arena_bytes)))
        self.rank, self.n_ranks = rank, n_ranks

    def peer_export(self):
        """(handle bytes for other processes, arena base address for contexts of this process)"""
        buf = C.create_string_buffer(_lib.MI_PEER_HANDLE_BYTES)
        base = vp()
        check(self._L.mi_ctx_peer_export(self._h, buf, C.byref(base)))
        return buf.raw, int(base.value or 0)

    def peer_import(self, rank: int, handle: bytes = None, same_process_base: int = 0) -> None:
        buf = C.create_string_buffer(handle, _lib.MI_PEER_HANDLE_BYTES) if handle is not None else None
        check(self._L.mi_ctx_peer_import(self._h, C.c_int(rank), buf, vp(same_process_base or None)))

    def peer_ready(self) -> None:
        check(self._L.mi_ctx_peer_ready(self._h))

    def set_exchange(self, mode) -> None:
        """`mi_ctx_set_exchange`: 0 / False — RCCL for everything; 1 / True — peer exchange, one-wave wait kernels between the
        launches; 2 — peer exchange, the folded launches wait for the flags themselves (only with one GPU per rank: a
        waiting launch keeps its compute units)."""
        check(self._L.mi_ctx_set_exchange(self._h, C.c_int(int(mode))))

    def query(self, what: str) -> int:
        """`mi_ctx_query`: "no_graph", "peer_exchange", "graph_replays", "exchanges", "spectral_pinv", "experimental", "folded_pcg",
        "graph_captures"."""
        out = i64(0)
        check(self._L.mi_ctx_query(self._h, C.c_int({"no_graph": 0, "peer_exchange": 1, "graph_replays": 2, "exchanges": 3, "spectral_pinv": 4, "experimental": 5, "folded_pcg": 6, "graph_captures": 7}[what]), C.byref(out)))
        return int(out.value)

    def peer_connect(self, rank: int, n_ranks: int, all_gather) -> None:
        """Whole hand-shake over any transport: `all_gather(obj) -> list of every rank's obj` (e.g. a wrapper of
        torch.distributed.all_gather_object)."""
        self.peer_init(rank, n_ranks)
        handle, _ = self.peer_export()
        handles = all_gather(handle)
        for q, h in enumerate(handles):
            if q != rank:
                self.peer_import(q, h)
        self.peer_ready()

    def allreduce_sum(self, v):
        self._mode_for(v)
        keep, p = self._ptr(v, writable=True)
        n = keep.numel() if _is_torch(keep) else keep.size
        check(self._L.mi_ctx_allreduce_sum(self._h, p, i64(n)))
        return keep

    # -- BLAS-1 (RecyclingKrylovSolvers.jl:3)
    def dot(self, x, y) -> float:
        self._mode_for(x, y)
        kx, px = self._ptr(x)
        n = kx.numel() if _is_torch(kx) else kx.size
        ky, py = self._ptr(y, n)
        out = C.c_double()
        check(self._L.mi_dot(self._h, i64(n), px, py, C.byref(out)))
        return out.value

    def norm2(self, x) -> float:
        self._mode_for(x)
        kx, px = self._ptr(x)
        n = kx.numel() if _is_torch(kx) else kx.size
        out = C.c_double()
        check(self._L.mi_norm2(self._h, i64(n), px, C.byref(out)))
        return out.value

    def axpy(self, a: float, x, y):
        """axpy!(a, x, y): y += a*x, returns y (numpy input: a new array unless y is writable fp64)."""
        self._mode_for(x, y)
        ky, py = self._ptr(y, writable=True)
        n = ky.numel() if _is_torch(ky) else ky.size
        kx, px = self._ptr(x, n)
        check(self._L.mi_axpy(self._h, i64(n), C.c_double(a), px, py))
        return ky

    def axpby(self, a: float, x, b: float, y):
        """axpby!(a, x, b, y): y = a*x + b*y."""
        self._mode_for(x, y)
        ky, py = self._ptr(y, writable=True)
        n = ky.numel() if _is_torch(ky) else ky.size
        kx, px = self._ptr(x, n)
        check(self._L.mi_axpby(self._h, i64(n), C.c_double(a), px, C.c_double(b), py))
        return ky

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.mi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LoopbackGroup:
    """`mi_loopback_group_create`: n in-process "ranks" (test facility, see include/mi355schur.h)."""

    def __init__(self, n: int):
        L = _lib.load()
        h = vp()
        check(L.mi_loopback_group_create(C.c_int(n), C.byref(h)))
        self._h, self._L, self.n = h, L, n

    def set_mode(self, mode: int) -> None:
        """0: device-side peer exchange when GPU_MAX_HW_QUEUES >= n (graphs); 1: host rendezvous (eager launches)."""
        check(self._L.mi_loopback_group_set_mode(self._h, C.c_int(mode)))

    def __del__(self):
        try:
            if self._h:
                self._L.mi_loopback_group_destroy(self._h)
                self._h = None
        except Exception:
            pass


class Event:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = vp()
        check(ctx._L.mi_event_create(C.byref(self._h)))

    def record(self) -> "Event":
        check(self.ctx._L.mi_event_record(self.ctx._h, self._h))
        return self

    def elapsed_ms(self, stop: "Event") -> float:
        out = C.c_double()
        check(self.ctx._L.mi_event_elapsed_ms(self._h, stop._h, C.byref(out)))
        return out.value

    def __del__(self):
        try:
            if self._h:
                self.ctx._L.mi_event_destroy(self._h)
                self._h = None
        except Exception:
            pass


class Operator:
    """`mi_op_t`: anything the solvers use through `A*x` / `mul!` or `M \\ r`."""

    def __init__(self, ctx: Context, handle, keep=()):
        self.ctx, self._h, self._keep = ctx, handle, keep
        n = i64()
        check(ctx._L.mi_op_size(handle, C.byref(n)))
        self.n = self.N = int(n.value)   # `.N` as LinearMaps.FunctionMap exposes it (Example07:273)

    def apply(self, x, out=None):
        self.ctx._mode_for(x, out)
        kx, px = self.ctx._ptr(x, self.n)
        if out is None:
            if _is_torch(kx):
                import torch
                out = torch.empty_like(kx)
            else:
                out = np.empty(self.n)
        ko, po = self.ctx._ptr(out, self.n, writable=True)
        self.ctx._order((kx, ko), after=False)
        check(self.ctx._L.mi_op_apply(self._h, px, po))
        self.ctx._order((kx, ko), after=True)
        return ko

    __call__ = apply
    __mul__ = apply          # A * x
    ldiv = apply             # M \ r  (`\` has no Python spelling)

    def bytes(self):
        a, d = i64(), i64()
        check(self.ctx._L.mi_op_bytes(self._h, C.byref(a), C.byref(d)))
        return int(a.value), int(d.value)

    def apply_dominant(self, x, reps: int = 1) -> None:
        self.ctx._mode_for(x)
        kx, px = self.ctx._ptr(x, self.n)
        check(self.ctx._L.mi_op_apply_dominant(self._h, px, C.c_int(reps)))

    def time_dominant(self, x, reps: int = 200) -> float:
        """Average microseconds per launch of the dominant kernel (HIP events, graph replay)."""
        self.ctx._mode_for(x)
        kx, px = self.ctx._ptr(x, self.n)
        out = C.c_double()
        check(self.ctx._L.mi_op_time_dominant(self._h, px, C.c_int(reps), C.byref(out)))
        return out.value

    def close(self) -> None:
        """`mi_op_destroy`. The library refuses it while a live `LorascPreconditioner` or `InterpolatingPreconditioner`
        borrows this operator: MiError, and the handle stays valid — close the borrower first. After `ctx.close()` nothing
        is called: the handles of a closed context are abandoned, not destroyed."""
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            check(self.ctx._L.mi_op_destroy(self._h))
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ operator constructors
def SparseMatrixCSC(ctx: Context, A, index_base: int = 0) -> Operator:
    """A symmetric `SparseMatrixCSC{Float64,Int}` as the solvers' `A` (cg.jl:14-15).
    `A` is a scipy sparse matrix or a (colptr, rowval, nzval, n) tuple."""
    if isinstance(A, tuple):
        ptr, idx, val, n = A
        ptr, idx, val = _i64(ptr), _i64(idx), _f64(val)
    else:
        A = sp.csr_matrix(A)
        A.sort_indices()
        n = A.shape[0]
        if A.shape[0] != A.shape[1]:
            raise ValueError("square matrix expected")
        ptr, idx, val = _i64(A.indptr), _i64(A.indices), _f64(A.data)
    h = vp()
    check(ctx._L.mi_csr_create(ctx._h, i64(n), i64(n), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                               val.ctypes.data_as(f64p), C.c_int(index_base), C.byref(h)))
    op = CsrOperator(ctx, h)
    op.nnz = int(val.size)
    return op


class CsrOperator(Operator):
    """What `SparseMatrixCSC` returns: the matrix operator, whose values can be replaced in place."""
    nnz = 0

    def set_values(self, A_or_nzval) -> None:
        """A new realization on the pattern of construction: a scipy sparse matrix, or its CSR values (sorted rows; the CSC
        values of a symmetric matrix) as a numpy array or a torch CUDA tensor (`mi_csr_set_values`). The values go into the
        same device array, so the solve graphs captured for this operator stay valid. A torch tensor is copied
        asynchronously on the context's stream."""
        v = A_or_nzval
        if sp.issparse(v):
            v = sp.csr_matrix(v)
            v.sum_duplicates()
            v.sort_indices()
            v = _f64(v.data)
        count = v.numel() if _is_torch(v) else np.size(v)
        if count != self.nnz:                       # the C call takes the length on trust: refused here, in its name
            raise MiError(_lib.MI_ERR_BAD_ARG, f"mi_csr_set_values: {count} values for {self.nnz} stored entries")
        self.ctx._mode_for(v)
        k, p = self.ctx._ptr(v, self.nnz)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_csr_set_values(self._h, p))
        self.ctx._record(k)


def IdentityPreconditioner(ctx: Context, n: int) -> Operator:
    h = vp()
    check(ctx._L.mi_diag_create(ctx._h, i64(n), None, C.byref(h)))
    return Operator(ctx, h)


def JacobiPreconditioner(ctx: Context, diag) -> Operator:
    """z = r ./ diag(A) — config 2's stand-in for Example01's AMG preconditioner (`AMGPreconditioner` is the V-cycle itself).
    `.refresh(A_op)` follows a matrix operator whose values have changed, on the device."""
    dinv = _f64(1.0 / np.asarray(diag, dtype=np.float64))
    h = vp()
    check(ctx._L.mi_diag_create(ctx._h, i64(dinv.size), dinv.ctypes.data_as(f64p), C.byref(h)))
    return JacobiOperator(ctx, h)


class JacobiOperator(Operator):
    """What `JacobiPreconditioner` returns."""

    def refresh(self, A: "CsrOperator") -> None:
        """dinv[r] = 1 / A[r, r] from the values the `SparseMatrixCSC` operator `A` holds now (`mi_diag_set_from_csr`): no
        host round trip, same device array (solve graphs stay valid). Synchronous."""
        check(self.ctx._L.mi_diag_set_from_csr(self._h, getattr(A, "_h", None)))


class SparseDirectPreconditioner(Operator):
    """`M \\ r` for a sparse SPD `M::SparseMatrixCSC` (cg.jl:85, 100): Example07:412/416 `pcg(S, b_schur, 0, A_ΓΓ)`.
    Exact, factored on the device by one level of nested dissection (`mi_spd_direct_create`). `A` is a scipy sparse matrix
    or a (colptr, rowval, nzval, n) tuple of CSC arrays; the pattern must be structurally symmetric. `.stats` =
    (pieces, |Σ|)."""

    def __init__(self, ctx: Context, A, index_base: int = 0):
        if isinstance(A, tuple):
            ptr, idx, val, n = A
            ptr, idx, val = _i64(ptr), _i64(idx), _f64(val)
        else:
            A = sp.csc_matrix(A)
            A.sum_duplicates()
            A.sort_indices()
            n = A.shape[0]
            if A.shape[0] != A.shape[1]:
                raise ValueError("square matrix expected")
            ptr, idx, val = _i64(A.indptr), _i64(A.indices), _f64(A.data)
        h = vp()
        check(ctx._L.mi_spd_direct_create(ctx._h, i64(n), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                                          val.ctypes.data_as(f64p), C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h)
        self.nnz = int(val.size)

    def set_values(self, nzval) -> None:
        """New values on the pattern of construction (CSC order): numpy array or torch CUDA tensor (`mi_spd_direct_set_values`)."""
        self.ctx._mode_for(nzval)
        k, p = self.ctx._ptr(nzval, self.nnz)
        self.ctx._order((k,), after=False)         # values made by torch kernels are complete before the factorisation reads them
        check(self.ctx._L.mi_spd_direct_set_values(self._h, p))   # synchronous

    @property
    def stats(self):
        a, b = i64(), i64()
        check(self.ctx._L.mi_spd_direct_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)


class BlockJacobiPreconditioner(Operator):
    """The reference's `BJPreconditioner(nb, A)` (MyPreconditioners/BJPreconditioner.jl:1-32) on the device
    (`mi_block_jacobi_create`): `M \\ r` solves the nb contiguous slices of `A` exactly, `bsize = n ÷ nb`, the last slice to
    the end. `A` is a scipy sparse matrix or a (colptr, rowval, nzval, n) tuple of CSC arrays with a structurally symmetric
    pattern. `seeds`: None for the default rule, or one array of block-local node indices per block (every connected
    component of a block needs one). `nb = 1` is `A \\ b`."""

    def __init__(self, ctx: Context, nb: int, A, seeds=None, index_base: int = 0):
        if isinstance(A, tuple):
            ptr, idx, val, n = A
            ptr, idx, val = _i64(ptr), _i64(idx), _f64(val)
        else:
            A = sp.csc_matrix(A)
            A.sum_duplicates()
            A.sort_indices()
            n = A.shape[0]
            if A.shape[0] != A.shape[1]:
                raise ValueError("square matrix expected")
            ptr, idx, val = _i64(A.indptr), _i64(A.indices), _f64(A.data)
        sq = sx = None
        if seeds is not None:
            if len(seeds) != nb:
                raise ValueError(f"{len(seeds)} seed lists for nb = {nb} blocks")
            sq = _i64(np.concatenate(([0], np.cumsum([len(s) for s in seeds]))) + index_base)
            sx = _i64(np.concatenate([np.asarray(s, dtype=np.int64).ravel() for s in seeds] + [np.zeros(0, dtype=np.int64)]))
            sx = _i64(np.concatenate((sx, [0])))          # never a NULL pointer for an empty list
        h = vp()
        check(ctx._L.mi_block_jacobi_create(ctx._h, i64(n), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                                            val.ctypes.data_as(f64p), i64(nb), None if sq is None else sq.ctypes.data_as(i64p),
                                            None if sx is None else sx.ctypes.data_as(i64p), C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h)
        self.nb, self.nnz = int(nb), int(val.size)

    def set_values(self, A_or_nzval) -> None:
        """A new realization on the pattern of construction: a scipy sparse matrix, or its CSC values as a numpy array or a
        torch CUDA tensor (`mi_block_jacobi_set_values`). MiError(MI_ERR_SINGULAR) leaves the previous factor in place.
        The test behind it is necessary, not sufficient: the elimination does not pivot and reports no pivots, so what is
        checked is that every value is finite, that every diagonal entry of every kept level inverse and of S_G^-1 is
        positive, and the probe certificate of S_G^-1. An indefinite matrix whose inverses all have positive diagonals is
        accepted (the same holds at construction)."""
        v = A_or_nzval
        if sp.issparse(v):
            v = sp.csc_matrix(v)
            v.sum_duplicates()
            v.sort_indices()
            v = _f64(v.data)
        self.ctx._mode_for(v)
        k, p = self.ctx._ptr(v, self.nnz)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_block_jacobi_set_values(self._h, p))   # synchronous

    def stats(self):
        """dict(n_g, n_levels, max_level: arrays of nb; kept_bytes = 8 Σ n_level²)"""
        a, b, c = (np.zeros(self.nb, dtype=np.int64) for _ in range(3))
        kb = i64()
        check(self.ctx._L.mi_block_jacobi_stats(self._h, a.ctypes.data_as(i64p), b.ctypes.data_as(i64p), c.ctypes.data_as(i64p),
                                                C.byref(kb)))
        return dict(n_g=a, n_levels=b, max_level=c, kept_bytes=int(kb.value))


class AMGPreconditioner(Operator):
    """The reference's `AMGPreconditioner{SmoothedAggregation}(A)` (Preconditioners.jl), the `Π_amg` of
    `pcg(A, b, zeros, Π_amg)` in Example01:49-61, on the device (`mi_amg_create`): `M \\ r` is one V(1,1) cycle of
    smoothed-aggregation AMG. `A_or_hierarchy`: a scipy sparse matrix — the set-up then runs here, on the host, with
    `fem.prepare_amg_precond(A, **kw)` (`max_levels`, `max_coarse`) — or a `fem.AmgHierarchy` built before. Usable as `M`
    of pcg / defpcg / eigpcg / eigdefpcg / initpcg and through `M * r`. Deviation from the reference: damped Jacobi where it
    smooths with symmetric Gauss-Seidel.

    `device_setup=True` (a matrix, not a hierarchy): `fem.prepare_amg_precond(A, **kw)` runs once, for the aggregates
    alone; the numbers of the hierarchy are made on the device (`mi_amg_plan_create`), and `.set_values(A_or_nzval)` redoes
    them for a new realization on the same pattern — the per-realization `Π_amg_t` of Example06:167-182 without a host
    set-up. The aggregates stay those of the first matrix: a later matrix with a different set of stored non-zeros gets
    a valid hierarchy, but not the one a fresh set-up would build. `aggregates=[agg_0, …]` (one 0-based array per smoothed
    level) skips the host set-up and freezes aggregates from elsewhere. Without `device_setup` a new matrix needs a new object.
    `.device_hierarchy()` reads the hierarchy back from the device (either kind)."""

    def __init__(self, ctx: Context, A_or_hierarchy, index_base: int = 0, device_setup: bool = False, **kw):
        H = A_or_hierarchy
        self.nnz = None
        if device_setup:
            if not (sp.issparse(H) or isinstance(H, np.ndarray)):
                raise TypeError("device_setup=True takes the matrix, not a hierarchy that is already built")
            from . import fem
            A = sp.csr_matrix(H)
            A.sum_duplicates()
            A.sort_indices()
            if "aggregates" in kw:        # frozen aggregates from elsewhere: one 0-based array per smoothed level
                H = None
                agg0 = [_i64(a).ravel() for a in kw.pop("aggregates")]
                if kw:
                    raise TypeError(f"set-up options {sorted(kw)} with aggregates that are already chosen")
                sizes = [A.shape[0]] + [int(a.max()) + 1 if a.size else 0 for a in agg0]
            else:
                H = fem.prepare_amg_precond(A, **kw)
                agg0, sizes = H.agg, H.sizes
            aggs = [_i64(a) + index_base for a in agg0]
            n_l = _i64(sizes)
            ptr, idx, val = _i64(A.indptr) + index_base, _i64(A.indices) + index_base, _f64(A.data)
            h = vp()
            check(ctx._L.mi_amg_plan_create(ctx._h, i64(A.shape[0]), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                                            val.ctypes.data_as(f64p), i64(len(sizes)), n_l.ctypes.data_as(i64p),
                                            _ptrs(aggs, i64p) if aggs else None, C.c_int(index_base), C.byref(h)))
            super().__init__(ctx, h)
            self.hierarchy = H            # of the matrix given here (None with `aggregates`); later values live on the device only
            self.aggregates = list(agg0)
            self.nnz = int(val.size)
            return
        if sp.issparse(H) or isinstance(H, np.ndarray):
            from . import fem
            H = fem.prepare_amg_precond(sp.csr_matrix(H), **kw)
        elif kw:
            raise TypeError(f"set-up options {sorted(kw)} with a hierarchy that is already built")
        L = H.nlevels
        n_l = _i64(H.sizes)

        def parts(mats):
            keep = []
            for M in mats:
                M = sp.csr_matrix(M)
                M.sort_indices()
                keep.append((_i64(M.indptr) + index_base, _i64(M.indices) + index_base, _f64(M.data)))
            return keep, _ptrs([k[0] for k in keep], i64p), _ptrs([k[1] for k in keep], i64p), _ptrs([k[2] for k in keep], f64p)

        ka, ap, ai, av = parts(H.A)
        kp, pp, pi, pv = parts(H.P)
        wd = _f64(np.concatenate([np.asarray(w, dtype=np.float64).ravel() for w in H.omega_over_d] + [np.zeros(1)]))
        inv = np.asfortranarray(H.coarse_inv, dtype=np.float64)
        nc = H.A[-1].shape[0]
        if inv.shape != (nc, nc) or len(H.A) != L or len(H.P) != L - 1 or len(H.omega_over_d) != L - 1:
            raise ValueError(f"coarse_inv is {inv.shape} for a coarsest level of {nc} rows, or the level lists do not fit {L} levels")
        if any(np.size(w) != a.shape[0] for w, a in zip(H.omega_over_d, H.A)):
            raise ValueError("omega_over_d: one entry per row of its level expected")
        h = vp()
        check(ctx._L.mi_amg_create(ctx._h, i64(L), n_l.ctypes.data_as(i64p), ap, ai, av, pp, pi, pv, wd.ctypes.data_as(f64p),
                                   inv.ctypes.data_as(f64p), C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h)
        self.hierarchy = H

    def set_values(self, A_or_nzval) -> None:
        """A new realization on the pattern of construction: a scipy sparse matrix, or its CSR values (sorted rows) as a numpy
        array or a torch CUDA tensor (`mi_amg_set_values`): the numeric chain of the hierarchy runs again on the device.
        Synchronous. MiError(MI_ERR_SINGULAR) — a diagonal entry of a level that is not positive, a value that is not finite,
        a coarse inverse that fails its certificate — leaves the previous hierarchy in place. Needs `device_setup=True`."""
        if self.nnz is None:
            raise TypeError("set_values needs AMGPreconditioner(ctx, A, device_setup=True); this hierarchy came from the host")
        v = A_or_nzval
        if sp.issparse(v):
            v = sp.csr_matrix(v)
            v.sum_duplicates()
            v.sort_indices()
            v = _f64(v.data)
        self.ctx._mode_for(v)
        k, p = self.ctx._ptr(v, self.nnz)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_amg_set_values(self._h, p))   # synchronous

    def refresh_profile(self) -> dict:
        """Milliseconds of the kernel groups of one refresh on the values held (`mi_amg_refresh_profile`, HIP events)."""
        ms = np.zeros(6)
        check(self.ctx._L.mi_amg_refresh_profile(self._h, ms.ctypes.data_as(f64p)))
        return dict(zip(("gershgorin_omega", "prolongator_R", "A_P", "R_AP_sym", "coarse_inverse", "commit"), (float(v) for v in ms)))

    def device_hierarchy(self):
        """The hierarchy as the device holds it, a `fem.AmgHierarchy` (`mi_amg_level_sizes`, `mi_amg_level_get`,
        `mi_amg_coarse_inverse`). `agg` is that of construction when known."""
        from . import fem
        L = self.ctx._L
        st = self.stats()
        As, Ps, om, owd = [], [], [], []
        for l in range(st["n_levels"]):
            n, m, an, pn = i64(), i64(), i64(), i64()
            check(L.mi_amg_level_sizes(self._h, i64(l), C.byref(n), C.byref(m), C.byref(an), C.byref(pn)))
            n, m, an, pn = int(n.value), int(m.value), int(an.value), int(pn.value)
            last = l == st["n_levels"] - 1
            ap, ai, av = np.zeros(n + 1, dtype=np.int64), np.zeros(an, dtype=np.int64), np.zeros(an)
            pp, pi, pv = np.zeros(n + 1, dtype=np.int64), np.zeros(pn, dtype=np.int64), np.zeros(pn)
            w, wd = C.c_double(0.0), np.zeros(n)
            check(L.mi_amg_level_get(self._h, i64(l), ap.ctypes.data_as(i64p), ai.ctypes.data_as(i64p), av.ctypes.data_as(f64p),
                                     pp.ctypes.data_as(i64p), pi.ctypes.data_as(i64p), pv.ctypes.data_as(f64p), C.byref(w),
                                     wd.ctypes.data_as(f64p)))   # (the P, ω outputs are left alone on the last level)
            As.append(sp.csr_matrix((av, ai, ap), shape=(n, n)))
            if not last:
                Ps.append(sp.csr_matrix((pv, pi, pp), shape=(n, m)))
                om.append(float(w.value)); owd.append(wd)
        nc = st["coarse_n"]
        inv = np.zeros((nc, nc), order="F")
        check(L.mi_amg_coarse_inverse(self._h, inv.ctypes.data_as(f64p)))
        nnz = [a.indices.size for a in As]
        return fem.AmgHierarchy(As, Ps, om, owd, inv, [a.shape[0] for a in As], float(sum(nnz)) / float(nnz[0]),
                                getattr(self, "aggregates", None) or getattr(self.hierarchy, "agg", None))

    def stats(self):
        """dict(n_levels, coarse_n, operator_nnz, bytes_kept) (`mi_amg_stats`)"""
        a, b, c, d = i64(), i64(), i64(), i64()
        check(self.ctx._L.mi_amg_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(n_levels=int(a.value), coarse_n=int(b.value), operator_nnz=int(c.value), bytes_kept=int(d.value))


class LorascPreconditioner(Operator):
    """The reference's `LorascPreconditioner` with `apply_lorasc` as its apply (EPDD.jl:1406-1428, 1908-1976): `M` of
    `pcg(A, b, zeros, ΠA_lorasc)` and `defpcg(A, b, zeros, ϕ, ΠA_lorasc)` on the full system (Example03:245-268), on the
    device (`mi_lorasc_create`).

    `A_IΓd`: the blocks of `prepare_global_schur` (Γ-global columns). `sub_or_maps`: where the unknowns sit in the rows of
    `A` — `(pos_I, pos_Γ)` (per subdomain the row of every interior node, and the row of every Γ node), or `(sub, dinds)`,
    or anything with `.sub` and `.dinds` (a `fem.SchurProblem`). `setup`: a `SchurSetup` of the same subdomains with
    `keep_levels()` and a `run()` after it (the exact `A_IId \\ f`); `A_ΓΓ_solver`: a `SparseDirectPreconditioner` of A_ΓΓ.
    Both are kept alive by this object and cannot be closed before it. `E` (n_Γ x nev) and `coef` (nev) are the low-rank
    correction x_Γ += Σ_k coef_k (E_k' z_Γ) E_k; `coef=None` is ones — the reference as written, whose loop never uses the
    Σ that `prepare_lorasc_precond` stores (EPDD.jl:1954-1957, 1596); pass `coef=Σ` for the correction of the paper."""

    def __init__(self, ctx: Context, A_IΓd, sub_or_maps, setup: "SchurSetup", A_ΓΓ_solver: "SparseDirectPreconditioner",
                 E=None, coef=None, index_base: int = 0):
        ndom, n_Γ, n_i, pI, pΓ, igp, igi, igv = _split_parts(
            A_IΓd, sub_or_maps, index_base, (), "one interior map per subdomain expected")
        nev, Ea, ca = _lorasc_correction(n_Γ, E, coef)
        h = vp()
        check(ctx._L.mi_lorasc_create(
            ctx._h, i64(ndom), i64(int(n_i.sum()) + n_Γ), i64(n_Γ), n_i.ctypes.data_as(i64p), _ptrs(pI, i64p),
            pΓ.ctypes.data_as(i64p), _ptrs(igp, i64p), _ptrs(igi, i64p), _ptrs(igv, f64p), setup._h, A_ΓΓ_solver._h, i64(nev),
            Ea.ctypes.data_as(f64p) if nev else None, ca.ctypes.data_as(f64p) if ca is not None else None,
            C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h, keep=(setup, A_ΓΓ_solver))
        self.setup, self.A_ΓΓ_solver = setup, A_ΓΓ_solver
        self.n_Γ, self.nev, self.nnz = n_Γ, nev, int(sum(v.size for v in igv))

    def set_values(self, ig_val) -> None:
        """The concatenated CSC `nzval` of all A_IΓd of a new realization: numpy array or torch CUDA tensor
        (`mi_lorasc_set_values`). The interior and A_ΓΓ factors move with `setup.run(...)` / `A_ΓΓ_solver.set_values(...)`."""
        _split_set_values(self, self.ctx._L.mi_lorasc_set_values, ig_val)

    def set_correction(self, E=None, coef=None) -> None:
        """A new low-rank correction (`mi_lorasc_set_correction`); `E=None` removes it."""
        nev, Ea, ca = _lorasc_correction(self.n_Γ, E, coef)
        self.ctx._mode_for(Ea)
        check(self.ctx._L.mi_lorasc_set_correction(self._h, i64(nev), vp(Ea.ctypes.data) if nev else None,
                                                   vp(ca.ctypes.data) if ca is not None else None))
        self.nev = nev

    def close(self) -> None:
        super().close()                 # before the plan and the A_ΓΓ solver it borrows
        self._keep = ()


def _lorasc_maps(sub_or_maps):
    if hasattr(sub_or_maps, "sub") and hasattr(sub_or_maps, "dinds"):
        sub_or_maps = (sub_or_maps.sub, sub_or_maps.dinds)
    a, b = sub_or_maps
    if hasattr(a, "node_Id") and hasattr(b, "not_dirichlet_g2l"):
        g2l = b.not_dirichlet_g2l
        return [g2l[nodes] for nodes in a.node_Id], g2l[a.node_Γ]
    return list(a), b


def _split_parts(A_IΓ, sub_or_maps, index_base: int, per_subdomain, complaint: str):
    """What both preconditioners on the interior/Γ split hand to the library: ndom, n_Γ, n_i, the two maps and the CSC
    arrays of the A_IΓ blocks in `index_base`; `per_subdomain`: further lists that must have one entry per subdomain."""
    pos_I, pos_Γ = _lorasc_maps(sub_or_maps)
    ndom = len(A_IΓ)
    if any(len(a) != ndom for a in (pos_I, *per_subdomain)):
        raise ValueError(complaint)
    n_i = _i64([len(p) for p in pos_I])
    pI = [_i64(p) + index_base for p in pos_I]
    pΓ = _i64(pos_Γ) + index_base
    return (ndom, int(pΓ.size), n_i, pI, pΓ) + _csc_parts(A_IΓ, 0, ndom, index_base)


def _split_set_values(op, entry, ig_val) -> None:
    op.ctx._mode_for(ig_val)
    k, p = op.ctx._ptr(ig_val, op.nnz)
    op.ctx._order((k,), after=False)
    check(entry(op._h, p))


def _lorasc_correction(n_Γ: int, E, coef):
    if E is None:
        return 0, np.empty(0), None
    Ea = np.asarray(E, dtype=np.float64)
    Ea = Ea.reshape(n_Γ, -1) if Ea.ndim == 1 else Ea
    if Ea.shape[0] != n_Γ:
        raise ValueError(f"E has {Ea.shape[0]} rows, n_Γ is {n_Γ}")
    nev = int(Ea.shape[1])
    Ea = np.ascontiguousarray(Ea.T).ravel()          # column-major n_Γ x nev
    ca = None
    if coef is not None and nev:
        ca = _f64(coef).ravel()
        if ca.size != nev:
            raise ValueError(f"coef has {ca.size} entries for {nev} vectors")
    return nev, Ea, ca


def _dom_slice(ctx: Context, ndom: int, dom_slice):
    if dom_slice is None:
        return shard_domains(ndom, ctx.rank, ctx.n_ranks)
    return int(dom_slice[0]), int(dom_slice[1])


def shard_domains(ndom: int, rank: int, n_ranks: int):
    """Contiguous block of subdomains owned by `rank` (8 subdomains: 8/4/2/1 per GPU at 1/2/4/8 GPUs)."""
    lo = ndom * rank // n_ranks
    hi = ndom * (rank + 1) // n_ranks
    return lo, hi


def _blocks(blocks, lo, hi):
    out = []
    for d, b in enumerate(blocks):
        out.append(np.asfortranarray(np.asarray(b, dtype=np.float64)) if (lo <= d < hi and b is not None) else None)
    return out


class LocalSchurs(Operator):
    """Assembled Schur operator: `x -> apply_local_schurs(Sd, ind_Γd_Γ2l, node_Γ_cnt, x)` (EPDD.jl:761-785),
    i.e. the closure Example03:131-135 wraps in a LinearMap."""

    def __init__(self, ctx: Context, Sd: Sequence, ind_Γd_Γ2l: Sequence, node_Γ_cnt, index_base: int = 0,
                 dom_slice=None):
        ndom = len(Sd)
        n_Γ = len(node_Γ_cnt)
        lo, hi = _dom_slice(ctx, ndom, dom_slice)
        g = [_i64(a) for a in ind_Γd_Γ2l]
        nd = _i64([a.size for a in g])
        S = _blocks(Sd, lo, hi)
        for d in range(lo, hi):
            if S[d].shape != (nd[d], nd[d]):
                raise ValueError(f"Sd[{d}] has shape {S[d].shape}, expected {(nd[d], nd[d])}")
        h = vp()
        check(ctx._L.mi_schur_assembled_create(ctx._h, i64(ndom), i64(n_Γ), nd.ctypes.data_as(i64p), _ptrs(g, i64p),
                                               _ptrs(S, f64p), C.c_int(index_base), i64(lo), i64(hi), C.byref(h)))
        super().__init__(ctx, h)
        self.dom_slice = (lo, hi)


class NeumannNeumannSchurPreconditioner(Operator):
    """`NeumannNeumannSchurPreconditioner(ΠSd, ind_Γd_Γ2l, node_Γ_cnt)` (EPDD.jl:1111-1137); used by the
    solvers through `Πnn \\ r` (EPDD.jl:1389-1392) = `apply_neumann_neumann_schur` (EPDD.jl:1361-1386).

    `storage="f32"` (or `numpy.float32`) holds the blocks as fp32 on the device: the apply is the fp64 apply of
    `ΠSd.astype(float32).astype(float64)`, half the bytes streamed; everything else stays fp64 (`mi_nn_create_stored`)."""

    _STORAGE = {"f64": 0, "f32": 1}

    def __init__(self, ctx: Context, ΠSd: Sequence, ind_Γd_Γ2l: Sequence, node_Γ_cnt, index_base: int = 0,
                 dom_slice=None, storage="f64"):
        if isinstance(storage, (type, np.dtype)):
            storage = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}.get(np.dtype(storage), storage)
        if storage not in self._STORAGE:
            raise ValueError(f"storage must be 'f64', 'f32', numpy.float64 or numpy.float32, not {storage!r}")
        ndom = len(ΠSd)
        cnt = _i64(node_Γ_cnt)
        lo, hi = _dom_slice(ctx, ndom, dom_slice)
        g = [_i64(a) for a in ind_Γd_Γ2l]
        nd = _i64([a.size for a in g])
        P = _blocks(ΠSd, lo, hi)
        h = vp()
        check(ctx._L.mi_nn_create_stored(ctx._h, i64(ndom), i64(cnt.size), nd.ctypes.data_as(i64p), _ptrs(g, i64p),
                                         _ptrs(P, f64p), cnt.ctypes.data_as(i64p), C.c_int(index_base), i64(lo), i64(hi),
                                         C.c_int(self._STORAGE[storage]), C.byref(h)))
        super().__init__(ctx, h)
        self.dom_slice = (lo, hi)

    @property
    def storage(self) -> str:
        """"f64" or "f32": the format the blocks are held in on the device (`mi_op_storage`)."""
        s = C.c_int()
        check(self.ctx._L.mi_op_storage(self._h, C.byref(s)))
        return "f32" if s.value == 1 else "f64"


class NeumannNeumannInducedPreconditioner(Operator):
    """The reference's `NeumannNeumannInducedPreconditioner` with `apply_neumann_neumann_induced` as its apply
    (EPDD.jl:2274-2285, 2363-2423): `M` of `defpcg(A, b, ϕ, M=ΠA_induced_nn_local_mat)` and
    `pcg(A, b, M=ΠA_induced_nn_local_mat)` on the full system (Example03:300-319), on the device (`mi_nn_induced_create`).

    `A_IΓdd`: the local blocks (n_Id x n_Γd, local columns) the set-up plan was created from. `sub_or_maps`: where the
    unknowns sit in the rows of `A` — `(pos_I, pos_Γ)`, or `(sub, dinds)`, or a `fem.SchurProblem`. `gather_idx`:
    `ind_Γd_Γ2l` as index arrays; `node_Γ_cnt`; `ΠSd`: the blocks of `prepare_neumann_neumann_induced_precond`. `setup`: a
    `SchurSetup` of the same subdomains with `keep_levels()` and a `run()` after it; it is kept alive by this object and
    cannot be closed before it. `storage`: "f64" or "f32", as for `NeumannNeumannSchurPreconditioner`.

    `coupling="reference"` is EPDD.jl:2411 as written: the interior is coupled to the local, unweighted, unassembled
    `z_Γd`, and the operator is neither symmetric nor positive definite (the reference's "only seems to work with
    deflation"). `coupling="assembled"` couples it to `z_Γ[gather_d]`: the symmetric positive definite block form."""

    _COUPLING = {"reference": _lib.MI_NNI_AS_WRITTEN, "assembled": _lib.MI_NNI_ASSEMBLED}

    def __init__(self, ctx: Context, A_IΓdd, sub_or_maps, gather_idx, node_Γ_cnt, ΠSd, setup: "SchurSetup", storage="f64",
                 coupling="reference", index_base: int = 0):
        if isinstance(storage, (type, np.dtype)):
            storage = {np.dtype(np.float64): "f64", np.dtype(np.float32): "f32"}.get(np.dtype(storage), storage)
        # (an unknown name goes to the library as it is, if it is a number: the library's message then names it)
        sto = NeumannNeumannSchurPreconditioner._STORAGE.get(storage, storage)
        cpl = self._COUPLING.get(coupling, coupling)
        if not isinstance(sto, (int, np.integer)):
            raise ValueError(f"storage must be 'f64', 'f32', numpy.float64 or numpy.float32, not {storage!r}")
        if not isinstance(cpl, (int, np.integer)):
            raise ValueError(f"coupling must be 'reference' or 'assembled', not {coupling!r}")
        ndom, n_Γ, n_i, pI, pΓ, igp, igi, igv = _split_parts(
            A_IΓdd, sub_or_maps, index_base, (gather_idx, ΠSd), "one interior map, one gather list and one ΠS_d block per subdomain expected")
        g = [_i64(a) + index_base for a in gather_idx]
        nd = _i64([a.size for a in g])
        cnt = _i64(node_Γ_cnt)
        blocks = _blocks(ΠSd, 0, ndom)
        for d in range(ndom):
            if blocks[d].shape != (nd[d], nd[d]):
                raise ValueError(f"ΠSd[{d}] has shape {blocks[d].shape}, expected {(nd[d], nd[d])}")
        h = vp()
        check(ctx._L.mi_nn_induced_create(
            ctx._h, i64(ndom), i64(int(n_i.sum()) + n_Γ), i64(n_Γ), nd.ctypes.data_as(i64p), n_i.ctypes.data_as(i64p),
            _ptrs(pI, i64p), pΓ.ctypes.data_as(i64p), _ptrs(g, i64p), cnt.ctypes.data_as(i64p), _ptrs(igp, i64p),
            _ptrs(igi, i64p), _ptrs(igv, f64p), _ptrs(blocks, f64p), C.c_int(int(sto)), setup._h, C.c_int(int(cpl)),
            C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h, keep=(setup,))
        self.setup = setup
        self.n_Γ, self.nnz, self.n_blocks = n_Γ, int(sum(v.size for v in igv)), int((nd * nd).sum())
        self.storage = "f32" if int(sto) == 1 else "f64"
        self.coupling = "assembled" if int(cpl) == _lib.MI_NNI_ASSEMBLED else "reference"

    def set_values(self, ig_val) -> None:
        """The concatenated CSC `nzval` of all A_IΓdd of a new realization: numpy array or torch CUDA tensor
        (`mi_nn_induced_set_values`). The interior factors move with `setup.run(...)`."""
        _split_set_values(self, self.ctx._L.mi_nn_induced_set_values, ig_val)

    def set_blocks(self, ΠSd) -> None:
        """New ΠS_d: one concatenated column-major buffer, numpy array or torch CUDA tensor (`mi_nn_induced_set_blocks`)."""
        self.ctx._mode_for(ΠSd)
        k, p = self.ctx._ptr(ΠSd, self.n_blocks)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_nn_induced_set_blocks(self._h, p))
        self.ctx._record(ΠSd)

    def set_coupling(self, coupling) -> None:
        """"reference" (EPDD.jl:2411 as written) or "assembled" (`mi_nn_induced_set_coupling`)."""
        cpl = self._COUPLING.get(coupling, coupling)
        if not isinstance(cpl, (int, np.integer)):
            raise ValueError(f"coupling must be 'reference' or 'assembled', not {coupling!r}")
        check(self.ctx._L.mi_nn_induced_set_coupling(self._h, C.c_int(int(cpl))))
        self.coupling = "assembled" if int(cpl) == _lib.MI_NNI_ASSEMBLED else "reference"

    def close(self) -> None:
        super().close()                 # before the plan it borrows
        self._keep = ()


def _wrap_interior(solvers: Sequence[Callable]):
    """`solvers[d](rhs) -> A_II[d]^{-1} rhs` on the host, as the C callback (EPDD.jl:648-650)."""
    def cb(_user, idom, n, rhs, sol):
        try:
            r = np.ctypeslib.as_array(rhs, shape=(n,))
            s = np.ctypeslib.as_array(sol, shape=(n,))
            s[:] = solvers[idom](r.copy())
            return 0
        except Exception:  # never let an exception cross the C frame
            return 1
    return _lib.INTERIOR_SOLVE_FN(cb)


def _csc_parts(mats, lo, hi, base: int = 0):
    """CSC arrays of the blocks lo..hi-1 as int64 in the `base` convention (1: what Julia's `colptr`/`rowval` hold)."""
    ptr, idx, val = [], [], []
    for d, m in enumerate(mats):
        if lo <= d < hi:
            m = sp.csc_matrix(m)
            m.sort_indices()
            ptr.append(_i64(m.indptr) + base); idx.append(_i64(m.indices) + base); val.append(_f64(m.data))
        else:
            ptr.append(None); idx.append(None); val.append(None)
    return ptr, idx, val


class _InteriorSolve:
    """What `MatrixFreeLocalSchurs` and `GlobalSchur` share: the calls built on the operator's interior solve (host callback,
    device interior CG or the level inverses of a `SchurSetup`) and the choice of that solve."""

    def schur_rhs(self, b_I, b_Γ):
        """`get_schur_rhs(b_Id, A_IIdd, A_IΓdd, b_Γ, ind_Γd_Γ2l; preconds)` (EPDD.jl:835-864) with this operator's
        interior solve; `b_I` is the concatenation of the b_Id of this operator's subdomains."""
        self.ctx._mode_for(b_I, b_Γ)
        k1, p1 = self.ctx._ptr(b_I)
        k2, p2 = self.ctx._ptr(b_Γ, self.n)
        if _is_torch(b_Γ):
            import torch
            out = torch.empty_like(b_Γ)
            po = vp(out.data_ptr())
        else:
            out = np.empty(self.n)
            po = vp(out.ctypes.data)
        self.ctx._order((k1, k2, out), after=False)
        check(self.ctx._L.mi_schur_matfree_rhs(self._h, p1, p2, po))
        self.ctx._order((k1, k2, out), after=True)
        return out

    def interior_solutions(self, u_Γ, b_I):
        """`get_subdomain_solutions(u_Γ, A_IId, A_IΓd, b_Id)` (EPDD.jl:1014-1025) with this operator's interior solve:
        the concatenation of u_Id = A_IIdd \\ (b_Id - A_IΓdd u_Γd) over this operator's subdomains."""
        self.ctx._mode_for(u_Γ, b_I)
        k1, p1 = self.ctx._ptr(u_Γ, self.n)
        k2, p2 = self.ctx._ptr(b_I)
        if _is_torch(b_I):
            import torch
            out = torch.empty_like(b_I)
            po = vp(out.data_ptr())
        else:
            out = np.empty(np.asarray(b_I).size)
            po = vp(out.ctypes.data)
        self.ctx._order((k1, k2, out), after=False)
        check(self.ctx._L.mi_schur_matfree_interior_solutions(self._h, p1, p2, po))
        self.ctx._order((k1, k2, out), after=True)
        return out

    def interior_precond(self, kind) -> None:
        """The `precond(s)` keyword of `apply_local_schur(s)` / `apply_global_schur` (EPDD.jl:648-650, 609-619) for the device
        interior CG: None / "none": plain CG (the default); "diagonal": `Pl = Diagonal(A_IIdd)`."""
        k = {None: 0, "none": 0, 0: 0, "diagonal": 1, "jacobi": 1, 1: 1}.get(kind)
        if k is None:
            raise ValueError("interior preconditioner: None or 'diagonal'")
        check(self.ctx._L.mi_schur_interior_precond(self._h, C.c_int(k)))

    def interior_iterations(self) -> int:
        """Diagnostic: iterations the device interior CG has run so far (slowest subdomain, rounded up to whole replays)."""
        out = i64(0)
        check(self.ctx._L.mi_schur_interior_iterations(self._h, C.byref(out)))
        return int(out.value)

    def interior_amg(self, A_IIdd=None, max_levels: int = 10, max_coarse: int = 256, sizes=None, aggregates=None, index_base: int = 0):
        """`Pl` = smoothed-aggregation AMG for the device interior CG (`mi_schur_interior_amg`): the reference's own `Pl`, the
        Π_IId of `IterativeSolvers.cg(A_IId, rhs; Pl = Π_IId, reltol)` (Example07:174). `A_IIdd`: the blocks the operator was
        made from — `fem.prepare_interior_amg(A_IIdd, max_levels, max_coarse)` aggregates their stacked pattern on the host,
        the numbers of the ONE hierarchy of blockdiag(A_IIdd) are made on the device from the operator's current values, and
        `set_values(ii_val=...)` redoes them for every realization. `sizes=, aggregates=` (0-based) instead of `A_IIdd` freeze
        aggregates from elsewhere; `index_base=1` sends them 1-based, as the Julia shim does. `interior_precond(None |
        "diagonal")` switches back and releases the hierarchy. Returns `interior_amg_stats()`."""
        if aggregates is None:
            if A_IIdd is None:
                raise TypeError("interior_amg: the blocks A_IIdd, or sizes= and aggregates=")
            from . import fem
            lo, hi = getattr(self, "_dom", (0, len(A_IIdd)))
            sizes, aggregates = fem.prepare_interior_amg(list(A_IIdd)[lo:hi], max_levels=max_levels, max_coarse=max_coarse)
        elif sizes is None:
            raise TypeError("interior_amg: aggregates= needs sizes= (the level sizes)")
        aggs = [_i64(a).ravel() + index_base for a in aggregates]
        n_l = _i64(sizes)
        if len(aggs) != len(n_l) - 1 or any(a.size != n for a, n in zip(aggs, n_l)):
            raise ValueError("interior_amg: one aggregate array per smoothed level, one id per node of the level")
        check(self.ctx._L.mi_schur_interior_amg(self._h, i64(len(n_l)), n_l.ctypes.data_as(i64p), _ptrs(aggs, i64p) if aggs else None,
                                                C.c_int(index_base)))
        return self.interior_amg_stats()

    def interior_amg_stats(self) -> dict:
        """dict(levels, coarse_n, bytes_kept) of the AMG `Pl` selected (`mi_schur_interior_amg_stats`)."""
        a, b, c = i64(), i64(), i64()
        check(self.ctx._L.mi_schur_interior_amg_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(levels=int(a.value), coarse_n=int(b.value), bytes_kept=int(c.value))

    def use_level_solver(self, setup: "SchurSetup" = None):
        """Interior solves of this matrix-free / global Schur operator through the level inverses `setup` keeps (exact, device;
        `mi_schur_matfree_interior_levels`); None: back to the operator's own callback / interior CG."""
        check(self.ctx._L.mi_schur_matfree_interior_levels(self._h, setup._h if setup is not None else None))
        self._level_setup = setup      # keep the plan alive


class MatrixFreeLocalSchurs(_InteriorSolve, Operator):
    """`x -> apply_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt, x; preconds, reltol)` (EPDD.jl:711-747),
    the closure of Example03:143-150. Sparse products on the device; `A_IIdd^{-1}` either through
    `interior_solvers[d](rhs)` on the host, or — `interior_solvers=None` — by the device CG that restates the
    reference's own `IterativeSolvers.cg(A_IIdd, rhs, reltol=reltol)` (EPDD.jl:648-650)."""

    def __init__(self, ctx: Context, A_IIdd, A_IΓdd, A_ΓΓdd, ind_Γd_Γ2l, node_Γ_cnt, interior_solvers=None,
                 reltol: float = 1e-9, dom_slice=None, index_base: int = 0):
        """`index_base=1`: `ind_Γd_Γ2l` holds 1-based Γ indices and the CSC arrays cross the ABI 1-based, exactly as the
        Julia shim passes `colptr`/`rowval` (the matrices themselves are scipy objects either way)."""
        ndom = len(A_IΓdd)
        n_Γ = len(node_Γ_cnt)
        lo, hi = _dom_slice(ctx, ndom, dom_slice)
        self._dom = (lo, hi)
        g = [_i64(a) for a in ind_Γd_Γ2l]
        nd = _i64([a.size for a in g])
        ni = _i64([A.shape[0] for A in A_IIdd])
        igp, igi, igv = _csc_parts(A_IΓdd, lo, hi, index_base)
        ggp, ggi, ggv = _csc_parts(A_ΓΓdd, lo, hi, index_base)
        h = vp()
        if interior_solvers is None:
            iip, iii, iiv = _csc_parts(A_IIdd, lo, hi, index_base)
            check(ctx._L.mi_schur_matfree_device_create(
                ctx._h, i64(ndom), i64(n_Γ), nd.ctypes.data_as(i64p), ni.ctypes.data_as(i64p), _ptrs(g, i64p),
                _ptrs(iip, i64p), _ptrs(iii, i64p), _ptrs(iiv, f64p), _ptrs(igp, i64p), _ptrs(igi, i64p), _ptrs(igv, f64p),
                _ptrs(ggp, i64p), _ptrs(ggi, i64p), _ptrs(ggv, f64p), C.c_double(reltol), C.c_int(index_base), i64(lo), i64(hi),
                C.byref(h)))
            super().__init__(ctx, h)
            return
        cb = _wrap_interior(interior_solvers)
        check(ctx._L.mi_schur_matfree_create(
            ctx._h, i64(ndom), i64(n_Γ), nd.ctypes.data_as(i64p), ni.ctypes.data_as(i64p), _ptrs(g, i64p),
            _ptrs(igp, i64p), _ptrs(igi, i64p), _ptrs(igv, f64p), _ptrs(ggp, i64p), _ptrs(ggi, i64p), _ptrs(ggv, f64p),
            cb, None, C.c_int(index_base), i64(lo), i64(hi), C.byref(h)))
        super().__init__(ctx, h, keep=(cb, interior_solvers))

    def set_values(self, ii_val=None, ig_val=None, gg_val=None) -> None:
        """New block values on the patterns given at construction (Example07:162-171 without re-creating the operator).
        Each argument: the concatenation over this operator's subdomains of the blocks' CSC `nzval` — the layout of
        `AssemblyPlan.run` / `fem.AssemblyPlan.layout` — as numpy arrays or torch CUDA tensors; None = unchanged."""
        self.ctx._mode_for(ii_val, ig_val, gg_val)
        k1, p1 = self.ctx._ptr(ii_val)
        k2, p2 = self.ctx._ptr(ig_val)
        k3, p3 = self.ctx._ptr(gg_val)
        check(self.ctx._L.mi_schur_matfree_set_values(self._h, p1, p2, p3))


class LocalSchur(MatrixFreeLocalSchurs):
    """`xd -> apply_local_schur(A_IIdd, A_IΓdd, A_ΓΓdd, xd; precond, reltol)` (EPDD.jl:639-654): ONE subdomain, vectors in
    its own Γ_d numbering — S_d xd = A_ΓΓdd xd - A_IΓdd' A_IIdd^{-1} (A_IΓdd xd). What `assemble_local_schurs` applies to the
    unit vectors (EPDD.jl:667-695) and `prepare_neumann_neumann_schur_precond` wraps (:1152-1189)."""

    def __init__(self, ctx: Context, A_IIdd, A_IΓdd, A_ΓΓdd, interior_solver=None, reltol: float = 1e-9,
                 index_base: int = 0):
        n = A_ΓΓdd.shape[0]
        super().__init__(ctx, [A_IIdd], [A_IΓdd], [A_ΓΓdd], [np.arange(n, dtype=np.int64) + index_base],
                         np.ones(n, dtype=np.int64), None if interior_solver is None else [interior_solver], reltol,
                         index_base=index_base)


class AssemblyPlan:
    """Device executor of a `fem.AssemblyPlan` (`mi_plan_t`): `run(a)` is the numeric half of
    `prepare_local_schurs(cells, points, epart, ..., a, f, uexact)` (EPDD.jl:389-546) for a new coefficient vector."""

    def __init__(self, ctx: Context, plan, index_base: int = 0):
        self.ctx, self.plan = ctx, plan
        h = vp()
        cells = _i64(plan.cells) + index_base      # index_base=1: node numbers as Julia's `cells` holds them
        arrs = [_f64(plan.G), _f64(plan.area), _f64(plan.ue), _f64(plan.be)]
        cptr, ccode = _i64(plan.cptr), _i64(plan.ccode)
        check(ctx._L.mi_assembly_plan_create(
            ctx._h, i64(cells.shape[1]), i64(plan.n_node), cells.ctypes.data_as(i64p), C.c_int(index_base),
            *[a.ctypes.data_as(f64p) for a in arrs], i64(plan.n_entries), i64(plan.n_matrix_entries),
            cptr.ctypes.data_as(i64p), ccode.ctypes.data_as(i64p), C.byref(h)))
        self._h = h

    def run(self, a_nodal):
        """values[n_entries]: numpy in -> numpy out; torch CUDA tensor in -> torch CUDA tensor out (stays on the device)."""
        self.ctx._mode_for(a_nodal)
        ka, pa = self.ctx._ptr(a_nodal, self.plan.n_node)
        if _is_torch(a_nodal):
            import torch
            out = torch.empty(self.plan.n_entries, dtype=torch.float64, device=a_nodal.device)
            po = vp(out.data_ptr())
        else:
            out = np.empty(self.plan.n_entries)
            po = vp(out.ctypes.data)
        check(self.ctx._L.mi_assembly_run(self._h, pa, po))
        self.ctx._record(a_nodal, out)
        return out

    def block_values(self, values, lo: int = 0, hi: Optional[int] = None):
        """(ii_val, ig_val, gg_val, b_I, b_Γ) slices of `values` for subdomains lo..hi-1: contiguous views, ready for
        `MatrixFreeLocalSchurs.set_values` / `.schur_rhs`."""
        L = self.plan.layout
        hi = len(L["II"]) if hi is None else hi

        def span(name):
            return values[L[name][lo][0]:L[name][hi - 1][0] + L[name][hi - 1][1]]
        off, cnt = L["bΓ"]
        return span("II"), span("IΓ"), span("ΓΓ"), span("bI"), values[off:off + cnt]

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx._L.mi_assembly_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FullAssemblyPlan:
    """Device executor of a `fem.FullAssemblyPlan` (`mi_full_assembly_plan_create`): the numeric half of
    `do_isotropic_elliptic_assembly(cells, points, dinds, point_marker, a, f, uexact)` (EllipticPde.jl:187-275) for a new
    nodal coefficient vector, bit for bit. `run(a) -> (values, b)` (CSR values of A on `plan.rowptr` / `plan.colidx`);
    `update(a, A_op) -> b` writes the values straight into a `SparseMatrixCSC` operator of that pattern — the reference's
    `update_isotropic_elliptic_assembly!` (:291-377)."""

    def __init__(self, ctx: Context, plan, index_base: int = 0):
        self.ctx, self.plan = ctx, plan
        h = vp()
        cells = _i64(plan.cells) + index_base      # index_base=1: node numbers as Julia's `cells` holds them
        rowptr, colidx = _i64(plan.rowptr) + index_base, _i64(plan.colidx) + index_base
        points, marker, ue, be = _f64(plan.points), _i64(plan.point_marker), _f64(plan.ue), _f64(plan.be)
        check(ctx._L.mi_full_assembly_plan_create(
            ctx._h, i64(cells.shape[1]), i64(plan.n_node), cells.ctypes.data_as(i64p), C.c_int(index_base),
            points.ctypes.data_as(f64p), marker.ctypes.data_as(i64p), i64(plan.n), rowptr.ctypes.data_as(i64p),
            colidx.ctypes.data_as(i64p), ue.ctypes.data_as(f64p), be.ctypes.data_as(f64p), C.byref(h)))
        self._h = h
        self.n, self.nnz = plan.n, plan.nnz

    def _b_like(self, a_nodal):
        if _is_torch(a_nodal):
            import torch
            return torch.empty(self.n, dtype=torch.float64, device=a_nodal.device)
        return np.empty(self.n)

    def run(self, a_nodal):
        """(values[nnz], b[n]): numpy in -> numpy out; torch CUDA tensor in -> torch CUDA tensors out (no host copy)."""
        self.ctx._mode_for(a_nodal)
        ka, pa = self.ctx._ptr(a_nodal, self.plan.n_node)
        b = self._b_like(ka)
        if _is_torch(ka):
            import torch
            values = torch.empty(self.nnz, dtype=torch.float64, device=ka.device)
        else:
            values = np.empty(self.nnz)
        _, pv = self.ctx._ptr(values, writable=True)
        _, pb = self.ctx._ptr(b, writable=True)
        self.ctx._order((ka,), after=False)
        check(self.ctx._L.mi_full_assembly_run(self._h, pa, pv, pb))
        self.ctx._record(ka, values, b)
        return values, b

    def update(self, a_nodal, A: "CsrOperator"):
        """b; the values of A(a) go into the device array of the operator `A` (its solve graphs stay valid)."""
        self.ctx._mode_for(a_nodal)
        ka, pa = self.ctx._ptr(a_nodal, self.plan.n_node)
        b = self._b_like(ka)
        _, pb = self.ctx._ptr(b, writable=True)
        self.ctx._order((ka,), after=False)
        check(self.ctx._L.mi_full_assembly_update(self._h, pa, getattr(A, "_h", None), pb))
        self.ctx._record(ka, b)
        return b

    def update_batch(self, a_nodal, batch: "CsrBatch", slot: int):
        """b; the values of A(a) go into slot `slot` of a `CsrBatch` of that pattern (`mi_full_assembly_update_batch`): the
        kernel and the bits of `update`."""
        self.ctx._mode_for(a_nodal)
        ka, pa = self.ctx._ptr(a_nodal, self.plan.n_node)
        b = self._b_like(ka)
        _, pb = self.ctx._ptr(b, writable=True)
        self.ctx._order((ka,), after=False)
        check(self.ctx._L.mi_full_assembly_update_batch(self._h, pa, getattr(batch, "_h", None), i64(int(slot)), pb))
        self.ctx._record(ka, b)
        return b

    def stats(self) -> dict:
        """dict(row_blocks, incidences, bytes_kept) (`mi_full_assembly_stats`)"""
        a, b, c = i64(), i64(), i64()
        check(self.ctx._L.mi_full_assembly_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(row_blocks=int(a.value), incidences=int(b.value), bytes_kept=int(c.value))

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx._L.mi_assembly_plan_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SchurSetup:
    """`assemble_local_schurs(A_IIdd, A_IΓdd, A_ΓΓdd, ...)` (EPDD.jl:667-695) on the device (`mi_setup_t`): built once from the
    blocks' sparsity, `run` per realization with the blocks' values — numpy arrays, or torch CUDA tensors as
    `AssemblyPlan.run` / `.block_values` leave them (nothing visits the host then)."""

    def __init__(self, ctx: Context, A_IIdd, A_IΓdd, A_ΓΓdd, index_base: int = 0):
        self.ctx = ctx
        ndom = len(A_IΓdd)
        self.n_Γd = [int(A.shape[0]) for A in A_ΓΓdd]
        self.n_Id = [int(A.shape[0]) for A in A_IIdd]
        nd, ni = _i64(self.n_Γd), _i64(self.n_Id)
        iip, iii, iiv = _csc_parts(A_IIdd, 0, ndom, index_base)
        igp, igi, igv = _csc_parts(A_IΓdd, 0, ndom, index_base)
        ggp, ggi, ggv = _csc_parts(A_ΓΓdd, 0, ndom, index_base)
        self._vals = (np.concatenate(iiv) if iiv else np.empty(0), np.concatenate(igv), np.concatenate(ggv))
        h = vp()
        check(ctx._L.mi_schur_setup_create(ctx._h, i64(ndom), nd.ctypes.data_as(i64p), ni.ctypes.data_as(i64p),
                                           _ptrs(iip, i64p), _ptrs(iii, i64p), _ptrs(igp, i64p), _ptrs(igi, i64p),
                                           _ptrs(ggp, i64p), _ptrs(ggi, i64p), C.c_int(index_base), C.byref(h)))
        self._h = h
        self.n_S = int(sum(n * n for n in self.n_Γd))
        self.n_w = int(sum(self.n_Γd))

    def run(self, ii_val=None, ig_val=None, gg_val=None, b_I=None):
        """-> (Sd, w): the concatenated column-major S_d blocks and (with b_I) the concatenated w_d = A_IΓdd' (A_IIdd \\ b_Id).
        Values default to those of the matrices given at construction."""
        ii_val = self._vals[0] if ii_val is None else ii_val
        ig_val = self._vals[1] if ig_val is None else ig_val
        gg_val = self._vals[2] if gg_val is None else gg_val
        self.ctx._mode_for(ii_val, ig_val, gg_val, b_I)
        k1, p1 = self.ctx._ptr(ii_val)
        k2, p2 = self.ctx._ptr(ig_val)
        k3, p3 = self.ctx._ptr(gg_val)
        k4, p4 = self.ctx._ptr(b_I)
        if _is_torch(ig_val):
            import torch
            Sd = torch.empty(self.n_S, dtype=torch.float64, device=ig_val.device)
            w = torch.empty(self.n_w, dtype=torch.float64, device=ig_val.device) if b_I is not None else None
            pS, pw = vp(Sd.data_ptr()), (vp(w.data_ptr()) if w is not None else None)
        else:
            Sd = np.empty(self.n_S)
            w = np.empty(self.n_w) if b_I is not None else None
            pS, pw = vp(Sd.ctypes.data), (vp(w.ctypes.data) if w is not None else None)
        check(self.ctx._L.mi_schur_setup_run(self._h, p1, p2, p3, p4, pS, pw))
        self.ctx._record(ii_val, ig_val, gg_val, b_I, Sd, w)
        return Sd, w

    def keep_levels(self, on: bool = True) -> None:
        """Every following `run` keeps the inverses of all elimination levels (`mi_schur_setup_keep_levels`): exact interior
        solves `interior_solve(f)` and `MatrixFreeLocalSchurs.use_level_solver(self)`."""
        check(self.ctx._L.mi_schur_setup_keep_levels(self._h, C.c_int(1 if on else 0)))

    def interior_solve(self, f):
        """u = A_IIdd \\ f for all subdomains (concatenated interior vectors, the order of b_I): exact, on the device."""
        self.ctx._mode_for(f)
        n = int(sum(self.n_Id))
        kf, pf = self.ctx._ptr(f, n)
        if _is_torch(f):
            import torch
            u = torch.empty_like(f)
            pu = vp(u.data_ptr())
        else:
            u = np.empty(n)
            pu = vp(u.ctypes.data)
        check(self.ctx._L.mi_schur_setup_interior_solve(self._h, pf, pu))
        self.ctx._record(f, u)
        return u

    def blocks(self, Sd):
        """The list of n_Γd x n_Γd column-major blocks of a concatenated buffer (views)."""
        out, off = [], 0
        for n in self.n_Γd:
            b = Sd[off:off + n * n]
            out.append(b.reshape(n, n).T if not _is_torch(Sd) else b.view(n, n).T)
            off += n * n
        return out

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx._L.mi_schur_setup_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nn_pinv(ctx: Context, n_Γd, Sd, rtol: float = 0.0):
    """`prepare_neumann_neumann_schur_precond(Sd, ...)`'s numeric half (EPDD.jl:1211): the concatenated ΠS_d = pinv(S_d,
    rtol = sqrt(eps)) of the concatenated symmetric blocks, on the device (`mi_nn_pinv`)."""
    nd = _i64(n_Γd)
    ctx._mode_for(Sd)
    k, p = ctx._ptr(Sd, int((nd * nd).sum()))
    if _is_torch(Sd):
        import torch
        out = torch.empty_like(Sd)
        po = vp(out.data_ptr())
    else:
        out = np.empty(k.size)
        po = vp(out.ctypes.data)
    check(ctx._L.mi_nn_pinv(ctx._h, i64(nd.size), nd.ctypes.data_as(i64p), p, C.c_double(rtol), po))
    ctx._record(Sd, out)
    return out


def device_dense_setup(ctx: Context):
    """`dense_setup` hook of `fem.build_schur_problem`: S_d, w_d (`assemble_local_schurs` + the condensed rhs of `get_schur_rhs`,
    EPDD.jl:667-695, 853-861) and ΠS_d (`prepare_neumann_neumann_schur_precond`, :1201-1220) from this library's device set-up
    (`mi_schur_setup_run`, `mi_nn_pinv`) — host arrays in and out."""
    def run(A_II, A_IΓ, A_ΓΓ, b_Id, want_pinv):
        setup = SchurSetup(ctx, A_II, A_IΓ, A_ΓΓ)
        Sd, w = setup.run(b_I=np.concatenate(b_Id))
        Sl = [np.asfortranarray(b) for b in setup.blocks(Sd)]
        wl, off = [], 0
        for n in setup.n_Γd:
            wl.append(w[off:off + n].copy())
            off += n
        Pl = [np.asfortranarray(b) for b in setup.blocks(nn_pinv(ctx, setup.n_Γd, Sd))] if want_pinv else None
        setup.close()
        return Sl, wl, Pl
    return run


def _set_blocks(self, blocks):
    """New S_d / ΠS_d (one concatenated column-major buffer, numpy or torch CUDA) on this operator's maps (`mi_dense_set_blocks`)."""
    self.ctx._mode_for(blocks)
    k, p = self.ctx._ptr(blocks)
    check(self.ctx._L.mi_dense_set_blocks(self._h, p))
    self.ctx._record(blocks)


LocalSchurs.set_blocks = _set_blocks
NeumannNeumannSchurPreconditioner.set_blocks = _set_blocks


class GlobalSchur(_InteriorSolve, Operator):
    """`x -> apply_global_schur(A_IId, A_IΓd, A_ΓΓ, x; preconds)` (EPDD.jl:596-625), the closure of Example03:101.
    `interior_solvers[d](rhs)` on the host, or — `interior_solvers=None` — the device CG that restates the reference's
    `IterativeSolvers.cg(A_IId[idom], A_IΓd[idom]*x)` (EPDD.jl:609-619; package default reltol = sqrt(eps))."""

    def __init__(self, ctx: Context, A_IId, A_IΓd, A_ΓΓ, interior_solvers=None, reltol: float = float(np.sqrt(np.finfo(float).eps)),
                 index_base: int = 0):
        ndom = len(A_IΓd)
        n_Γ = A_ΓΓ.shape[0]
        ni = _i64([A.shape[0] for A in A_IId])
        igp, igi, igv = _csc_parts(A_IΓd, 0, ndom, index_base)
        (ggp,), (ggi,), (ggv,) = _csc_parts([A_ΓΓ], 0, 1, index_base)
        h = vp()
        if interior_solvers is None:
            iip, iii, iiv = _csc_parts(A_IId, 0, ndom, index_base)
            check(ctx._L.mi_schur_global_device_create(
                ctx._h, i64(ndom), i64(n_Γ), ni.ctypes.data_as(i64p), _ptrs(iip, i64p), _ptrs(iii, i64p), _ptrs(iiv, f64p),
                _ptrs(igp, i64p), _ptrs(igi, i64p), _ptrs(igv, f64p), ggp.ctypes.data_as(i64p), ggi.ctypes.data_as(i64p),
                ggv.ctypes.data_as(f64p), C.c_double(reltol), C.c_int(index_base), C.byref(h)))
            super().__init__(ctx, h)
            return
        cb = _wrap_interior(interior_solvers)
        check(ctx._L.mi_schur_global_create(
            ctx._h, i64(ndom), i64(n_Γ), ni.ctypes.data_as(i64p), _ptrs(igp, i64p), _ptrs(igi, i64p), _ptrs(igv, f64p),
            ggp.ctypes.data_as(i64p), ggi.ctypes.data_as(i64p), ggv.ctypes.data_as(f64p), cb, None, C.c_int(index_base), C.byref(h)))
        super().__init__(ctx, h, keep=(cb, interior_solvers))


# reference-named free functions
def apply_local_schur(S_d: LocalSchur, xd):
    return S_d.apply(xd)


def apply_local_schurs(S: Operator, x):
    return S.apply(x)


def apply_global_schur(S: GlobalSchur, x):
    return S.apply(x)


def apply_neumann_neumann_schur(Πnn: NeumannNeumannSchurPreconditioner, r):
    return Πnn.apply(r)


def apply_lorasc(Πlorasc: LorascPreconditioner, x):
    return Πlorasc.apply(x)


def apply_neumann_neumann_induced(Πnn: NeumannNeumannInducedPreconditioner, r):
    return Πnn.apply(r)


def apply_amg(Π_amg: AMGPreconditioner, r):
    """`Π_amg \\ r`: one V-cycle"""
    return Π_amg.apply(r)


# ------------------------------------------------------------------ solvers
def _solve(kind: str, A: Operator, M: Optional[Operator], b, x, W, maxit: int, eps: float, nvec_out: int = 0,
           spdim: int = 0):
    ctx = A.ctx
    n = A.n
    ctx._mode_for(b, x, W)
    kb, pb = ctx._ptr(b, n)
    if _is_torch(x):
        kx, px = ctx._ptr(x, n, writable=True)       # mutated in place like the reference's x
    else:
        kx = np.array(x, dtype=np.float64, copy=True)
        if kx.size != n:
            raise ValueError(f"expected {n} entries, got {kx.size}")
        px = vp(kx.ctypes.data)
    cap = int(min(maxit if maxit else n, n)) + 1
    res, res_p = ctx._res_buffer(cap)
    it = i64()
    L = ctx._L
    tail = (maxit, eps, res_p, cap, C.byref(it))
    if W is not None:
        if _is_torch(W):
            if W.dim() != 2 or W.shape[0] != n or W.stride(0) != 1:
                raise TypeError("W must be an n x nvec column-major tensor (e.g. torch.empty(nvec, n).T)")
            nvec, kW, pW = W.shape[1], W, vp(W.data_ptr())
        else:
            kW = np.asfortranarray(W, dtype=np.float64)
            if kW.ndim != 2 or kW.shape[0] != n:
                raise ValueError("W must be n x nvec")
            nvec, pW = kW.shape[1], vp(kW.ctypes.data)
    V = pV = None
    if kind.startswith("eig"):
        nv = nvec if W is not None else int(nvec_out)
        # V[:, 1:nvec] comes back where x lives: a column-major torch tensor on the device, or a Fortran numpy array
        if _is_torch(x):
            import torch
            V = torch.empty((nv, n), dtype=torch.float64, device=x.device).T
            pV = vp(V.data_ptr())
        else:
            V = np.empty((n, nv), order="F")
            pV = vp(V.ctypes.data)
    if kind == "cg":
        rc = L.mi_cg(A._h, pb, px, *tail)
    elif kind == "pcg":
        rc = L.mi_pcg(A._h, M._h, pb, px, *tail)
    elif kind == "defcg":
        rc = L.mi_defcg(A._h, pb, px, pW, i64(nvec), *tail)
    elif kind == "defpcg":
        rc = L.mi_defpcg(A._h, M._h, pb, px, pW, i64(nvec), *tail)
    elif kind == "initcg":
        rc = L.mi_initcg(A._h, pb, px, pW, i64(nvec), *tail)
    elif kind == "initpcg":
        rc = L.mi_initpcg(A._h, M._h, pb, px, pW, i64(nvec), *tail)
    elif kind == "eigcg":
        rc = L.mi_eigcg(A._h, pb, px, i64(nvec_out), i64(spdim), *tail, pV)
    elif kind == "eigpcg":
        rc = L.mi_eigpcg(A._h, M._h, pb, px, i64(nvec_out), i64(spdim), *tail, pV)
    elif kind == "eigdefcg":
        rc = L.mi_eigdefcg(A._h, pb, px, pW, i64(nvec), i64(spdim), *tail, pV)
    elif kind == "eigdefpcg":
        rc = L.mi_eigdefpcg(A._h, M._h, pb, px, pW, i64(nvec), i64(spdim), *tail, pV)
    else:
        raise ValueError(kind)
    try:
        check(rc)
    except BoundsError as e:   # the reference mutates x in place before `res_norm[it]` throws: hand the state over
        e.x, e.it = kx, int(it.value)
        raise
    k = int(it.value)
    if V is not None:
        return kx, k, res[:k].copy(), V
    return kx, k, res[:k].copy()


def cg(A: Operator, b, x, maxit: int = 0, eps: float = EPS):
    """cg(A, b, x; maxit=0) (cg.jl:14-50)."""
    return _solve("cg", A, None, b, x, None, maxit, eps)


def pcg(A: Operator, b, x, M: Operator, maxit: int = 0, eps: float = EPS):
    """pcg(A, b, x, M; maxit=0) (cg.jl:67-109)."""
    return _solve("pcg", A, M, b, x, None, maxit, eps)


def defcg(A: Operator, b, x, W, maxit: int = 0, eps: float = EPS):
    """defcg(A, b, x, W; maxit=0) (defcg.jl:24-83)."""
    return _solve("defcg", A, None, b, x, W, maxit, eps)


def defpcg(A: Operator, b, x, W, M: Operator, maxit: int = 0, eps: float = EPS):
    """defpcg(A, b, x, W, M; maxit=0) (defcg.jl:242-308) — note the reference's (A,b,x,W,M) order."""
    return _solve("defpcg", A, M, b, x, W, maxit, eps)


def eigcg(A: Operator, b, x, nvec: int, spdim: int, maxit: int = 0, eps: float = EPS):
    """eigcg(A, b, x, nvec, spdim; maxit=0) -> (x, it, res_norm, V[:, 1:nvec]) (eigcg.jl:27-123)."""
    return _solve("eigcg", A, None, b, x, None, maxit, eps, nvec, spdim)


def eigpcg(A: Operator, b, x, M: Operator, nvec: int, spdim: int, maxit: int = 0, eps: float = EPS):
    """eigpcg(A, b, x, M, nvec, spdim; maxit=0) -> (x, it, res_norm, V[:, 1:nvec]) (eigcg.jl:143-290)."""
    return _solve("eigpcg", A, M, b, x, None, maxit, eps, nvec, spdim)


def eigdefcg(A: Operator, b, x, W, spdim: int, maxit: int = 0, eps: float = EPS):
    """eigdefcg(A, b, x, W, spdim; maxit=0) -> (x, it, res_norm, V[:, 1:nvec]) (defcg.jl:111-223)."""
    return _solve("eigdefcg", A, None, b, x, W, maxit, eps, 0, spdim)


def eigdefpcg(A: Operator, b, x, M: Operator, W, spdim: int, maxit: int = 0, eps: float = EPS):
    """eigdefpcg(A, b, x, M, W, spdim; maxit=0) -> (x, it, res_norm, V[:, 1:nvec]) (defcg.jl:337-473) — (A,b,x,M,W) order."""
    return _solve("eigdefpcg", A, M, b, x, W, maxit, eps, 0, spdim)


def initcg(A: Operator, b, x, W, maxit: int = 0, eps: float = EPS):
    """initcg(A, b, x, W; maxit=0) (initcg.jl:28-75)."""
    return _solve("initcg", A, None, b, x, W, maxit, eps)


def initpcg(A: Operator, b, x, M: Operator, W, maxit: int = 0, eps: float = EPS):
    """initpcg(A, b, x, M, W; maxit=0) (initcg.jl:106-160)."""
    return _solve("initpcg", A, M, b, x, W, maxit, eps)



# ------------------------------------------------------------------ eigensolver
class ConvergenceInfo:
    """KrylovKit's `ConvergenceInfo` by its field names: `converged` (leading pairs with normres <= tol), `normres` (the
    residual estimates of the returned pairs), `numiter` (restarts), `numops` (applies of A)."""

    def __init__(self, converged: int, normres, numiter: int, numops: int):
        self.converged, self.normres, self.numiter, self.numops = converged, normres, numiter, numops

    def __repr__(self):
        return f"ConvergenceInfo(converged={self.converged}, numiter={self.numiter}, numops={self.numops}, normres={self.normres})"


_WHICH = {"SR": _lib.MI_EIG_SR, "LR": _lib.MI_EIG_LR}


def _eigsolve(A: Operator, B: Optional[Operator], Binv: Optional[Operator], nev: int, which, krylovdim: int, tol: float,
              maxiter: int, v0):
    ctx, n = A.ctx, A.n
    if which not in _WHICH:
        raise ValueError(f"which = {which!r}: 'SR' or 'LR' expected")
    nev = int(nev)
    ctx._mode_for(v0)
    k0, p0 = ctx._ptr(v0, n)
    if _is_torch(v0):
        import torch
        vecs = torch.empty((max(nev, 0), n), dtype=torch.float64, device=v0.device).T
        pv = vp(vecs.data_ptr())
    else:
        vecs = np.empty((n, max(nev, 0)), order="F")
        pv = vp(vecs.ctypes.data)
    vals, res = np.empty(max(nev, 1)), np.empty(max(nev, 1))
    nconv, nrestart, napply = i64(), i64(), i64()
    ctx._order((k0, vecs), after=False)
    check(ctx._L.mi_eigsolve(A._h, B._h if B is not None else None, Binv._h if Binv is not None else None, i64(nev),
                             C.c_int(_WHICH[which]), i64(krylovdim), C.c_double(tol), i64(maxiter), p0,
                             vals.ctypes.data_as(f64p), pv, res.ctypes.data_as(f64p), C.byref(nconv), C.byref(nrestart),
                             C.byref(napply)))
    ctx._order((k0, vecs), after=True)
    return vals[:nev], vecs, ConvergenceInfo(int(nconv.value), res[:nev], int(nrestart.value), int(napply.value))


def eigsolve(A: Operator, nev: int, which: str = "SR", krylovdim: int = 0, tol: float = 1e-12, maxiter: int = 100, v0=None):
    """KrylovKit.eigsolve(x -> A*x, n, nev, :SR | :LR, krylovdim=...) (Example03:209/219) -> (vals, vecs, info): thick-restart
    Lanczos on the device (`mi_eigsolve`). `vecs` is n x nev with orthonormal columns; `tol` is absolute."""
    return _eigsolve(A, None, None, nev, which, krylovdim, tol, maxiter, v0)


def geneigsolve(A: Operator, B: Operator, Binv: Operator, nev: int, which: str = "SR", krylovdim: int = 0, tol: float = 1e-12,
                maxiter: int = 100, v0=None):
    """KrylovKit.geneigsolve(x -> (A*x, B*x), n, nev, :SR, krylovdim=..., isposdef=true) (EPDD.jl:1546-1549) -> (vals, vecs, info)
    with vecs' B vecs = I. `Binv` applies the exact inverse of the SPD `B` (e.g. SparseDirectPreconditioner(ctx, A_ΓΓ))."""
    return _eigsolve(A, B, Binv, nev, which, krylovdim, tol, maxiter, v0)


# ------------------------------------------------------------------ Karhunen-Loève on the matrix-free covariance kernel
_COV_MODEL = {"SExp": _lib.MI_COV_SEXP, "Exp": _lib.MI_COV_EXP}


def _cov_model(model) -> int:
    if model not in _COV_MODEL:
        raise ValueError(f"model = {model!r}: 'SExp' or 'Exp' expected")
    return _COV_MODEL[model]


def _points_2xn(points):
    """(2, n) coordinates -> the reference's `points` layout in memory (x and y of a node adjacent) and n."""
    p = np.asarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] != 2:
        raise ValueError("points: a (2, n) array expected")
    return np.ascontiguousarray(p.T), p.shape[1]


def cov_tiling(nt: int, ns: int, m: int = 1):
    """`mi_cov_tiling` -> (row_tile, src_chunk, col_block, splits); a pure host function, no device needed."""
    out = [i64() for _ in range(4)]
    check(_lib.load().mi_cov_tiling(i64(nt), i64(ns), i64(m), *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def cov_apply(ctx: Context, model: str, sig2: float, L: float, pt, ps, X):
    """Y = K(pt, ps) X with K[i, j] = cov(pt[:, i], ps[:, j]) evaluated on the fly (`mi_cov_apply`): the covariance
    evaluations of KarhunenLoeve.jl:75-77 / KLDD.jl:508-547 applied to a vector (ns,) or a panel (ns, m). numpy arrays."""
    pt_m, nt = _points_2xn(pt)
    ps_m, ns = (pt_m, nt) if ps is pt else _points_2xn(ps)
    X = np.asarray(X, dtype=np.float64)
    vec = X.ndim == 1
    Xf = np.asfortranarray(X.reshape(ns, -1))
    m = Xf.shape[1]
    Y = np.empty((nt, m), order="F")
    check(ctx._L.mi_ctx_set_pointer_mode(ctx._h, _lib.MI_PTR_HOST))
    check(ctx._L.mi_cov_apply(ctx._h, C.c_int(_cov_model(model)), C.c_double(sig2), C.c_double(L), i64(nt), vp(pt_m.ctypes.data),
                              i64(ns), vp(ps_m.ctypes.data), i64(m), vp(Xf.ctypes.data), i64(ns), vp(Y.ctypes.data), i64(nt)))
    return Y[:, 0].copy() if vec else Y


class CovarianceOperator(Operator):
    """x -> C x with C = M K M, K[i, j] = cov(p_i, p_j): the dense matrix of do_mass_covariance_assembly
    (KarhunenLoeve.jl:27-108; local form KLDD.jl:120-204) as a matrix-free operator (`mi_kl_cov_create`). `M`: the mass
    matrix of the same nodes (scipy sparse, symmetric)."""

    def __init__(self, ctx: Context, points, M, model: str = "SExp", sig2: float = 1.0, L: float = 0.1):
        pts, n = _points_2xn(points)
        M = sp.csr_matrix(M)
        M.sort_indices()
        if M.shape != (n, n):
            raise ValueError(f"M is {M.shape}, {n} nodes")
        ptr, idx, val = _i64(M.indptr), _i64(M.indices), _f64(M.data)
        h = vp()
        check(ctx._L.mi_kl_cov_create(ctx._h, C.c_int(_cov_model(model)), C.c_double(sig2), C.c_double(L), i64(n),
                                      pts.ctypes.data_as(f64p), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p),
                                      val.ctypes.data_as(f64p), C.byref(h)))
        super().__init__(ctx, h)
        self.model, self.sig2, self.L = model, sig2, L


def _kl_pairs(ctx: Context, points, M, nev: int, model, sig2, L, tol, maxiter):
    """`Arpack.eigs(C, M, nev=nev)` (KarhunenLoeve.jl:138, KLDD.jl:679): the nev dominant pairs of C ϕ = λ M ϕ with Φ' M Φ = I,
    krylovdim = Arpack's default ncv = max(20, 2 nev + 1)."""
    Cop = CovarianceOperator(ctx, points, M, model, sig2, L)
    Mop = SparseMatrixCSC(ctx, M)
    Minv = None
    try:
        Minv = SparseDirectPreconditioner(ctx, M)
    except MiError as e:                           # a separator above the one-level dissection's cap (n in the tens of thousands)
        if e.code != _lib.MI_ERR_BAD_ARG:
            raise
        Minv = BlockJacobiPreconditioner(ctx, 1, M)   # nb = 1 is `M \ b`, exact, by breadth-first level elimination
    try:
        λ, Φ, info = geneigsolve(Cop, Mop, Minv, nev, "LR", krylovdim=max(20, 2 * nev + 1), tol=tol, maxiter=maxiter)
    finally:
        Cop.close()
        Mop.close()
        Minv.close()
    if info.converged < nev:                       # Arpack throws where its iteration does not converge; so does this
        raise RuntimeError(f"solve_kl: {info.converged} of {nev} pairs converged to {tol:g} in {maxiter} restarts")
    return np.array(λ), np.asfortranarray(Φ), info


def solve_kl(ctx: Context, cells, points, nev: int, model: str = "SExp", sig2: float = 1.0, L: float = 0.1, relative: float = 0.99,
             tol: float = 1e-12, maxiter: int = 100, verbose: bool = True):
    """`solve_kl(cells, points, cov, nev; relative)` (KarhunenLoeve.jl:123-193) -> (Λ[:nvec], Φ[:, :nvec]): the dominant pairs
    of C ϕ = λ M ϕ on the device, then the reference's keep loop: positive eigenvalues until relative · Area · cov(centre,
    centre) is reached."""
    from . import fem
    M = fem.get_mass_matrix(cells, points)
    λ, Φ, _ = _kl_pairs(ctx, points, M, nev, model, sig2, L, tol, maxiter)
    Area, center = fem.kl_energy(cells, points)
    energy_expected = relative * Area * float(fem.cov(model, center[0], center[1], center[0], center[1], sig2, L))
    nvec, energy_achieved = fem.kl_keep(λ, energy_expected)
    if verbose:
        print(f"{nvec}/{nev} vectors kept for {energy_achieved / energy_expected * relative:.5f} relative energy")
    return λ[:nvec], Φ[:, :nvec]


def solve_local_kl(ctx: Context, cells, points, epart, nev: int, idom: int, model: str = "SExp", sig2: float = 1.0, L: float = 0.1,
                   relative: float = 0.99, tol: float = 1e-12, maxiter: int = 100, verbose: bool = True):
    """`solve_local_kl(cells, points, epart, cov, nev, idom; relative)` (KLDD.jl:657-735) -> fem.KLSubDomain: the same on the
    nodes and elements of subdomain `idom` (0-based)."""
    from . import fem
    inds_l2g, inds_g2l, elems, center = fem.kl_set_subdomain(cells, points, epart, idom)
    M = fem.do_local_mass_assembly(cells, points, inds_g2l, elems)
    λ, Φ, _ = _kl_pairs(ctx, points[:, inds_l2g], M, nev, model, sig2, L, tol, maxiter)
    Area, _ = fem.kl_energy(cells, points, elems)
    energy_expected = relative * Area * float(fem.cov(model, center[0], center[1], center[0], center[1], sig2, L))
    nvec, energy_achieved = fem.kl_keep(λ, energy_expected)
    if verbose:
        print(f"idom = {idom}, {nvec}/{nev} vectors kept for {energy_achieved / energy_expected * relative:.5f} relative energy")
    return fem.KLSubDomain(inds_g2l, inds_l2g, elems, Φ[:, :nvec], center, energy_expected / relative, M, λ)


def do_global_mass_covariance_reduced_assembly(ctx: Context, points, subdomains, Φd, centerd, model: str = "SExp", sig2: float = 1.0,
                                               L: float = 0.1, forget: float = -1.0):
    """`do_global_mass_covariance_reduced_assembly` (KLDD.jl:465-614) -> K (Σ md x Σ md): for every pair idom <= jdom whose
    centre covariance exceeds `forget`, block (idom, jdom) = Φ_i' (M_i (K(P_i, P_j) (M_j Φ_j))) with the covariance panel
    product on the device — the dense C[i, j] of KLDD.jl:505-586 is M_i K(P_i, P_j) M_j and is never formed. The mirror block
    is copied (KLDD.jl:604); a diagonal block is mirrored from its upper triangle, the half `Symmetric(K)` reads (KLDD.jl:791).
    `subdomains`: objects with `.inds_l2g` and `.M` (fem.KLSubDomain)."""
    from . import fem
    md = [int(np.asarray(Φ).shape[1]) for Φ in Φd]
    off = np.concatenate([[0], np.cumsum(md)]).astype(int)
    K = np.zeros((off[-1], off[-1]))
    P = [np.asarray(points)[:, s.inds_l2g] for s in subdomains]
    MΦ = [np.asfortranarray(s.M @ np.asarray(Φ)) for s, Φ in zip(subdomains, Φd)]
    for idom in range(len(Φd)):
        for jdom in range(idom, len(Φd)):
            ci, cj = centerd[idom], centerd[jdom]
            if not float(fem.cov(model, ci[0], ci[1], cj[0], cj[1], sig2, L)) > forget:
                continue
            Z = cov_apply(ctx, model, sig2, L, P[idom], P[jdom], MΦ[jdom])
            blk = MΦ[idom].T @ Z                                  # Φ_i' M_i Z (M_i is symmetric)
            if idom == jdom:
                blk = np.triu(blk) + np.triu(blk, 1).T
            K[off[idom]:off[idom + 1], off[jdom]:off[jdom + 1]] = blk
            if idom != jdom:
                K[off[jdom]:off[jdom + 1], off[idom]:off[idom + 1]] = blk.T
    return K


# ------------------------------------------------------------------ realization sampler: ξ -> g -> a = exp(g)
def kl_field_tiling(n: int, m: int, nreal: int = 1):
    """`mi_kl_field_tiling` -> (row_tile, mode_chunk, real_block, coord_splits); a pure host function, no device needed."""
    out = [i64() for _ in range(4)]
    check(_lib.load().mi_kl_field_tiling(i64(n), i64(m), i64(nreal), *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


class KLField:
    """Device form of the step from a latent vector to the field and the coefficient (`mi_kl_field_t`): `set(ξ)` is
    `set!(Λ, Ψ, ξ, g)` (KLDD.jl:1150-1164) / the field half of `draw!` (KLDD.jl:1037-1040, Samplers.jl:64-67), `coefficient(ξ)`
    is `exp.(g)`. `KLField(ctx, Λ, Ψ)` keeps Ψ (n x m) on the device; `KLField.from_dd` keeps the factors of
    `draw(mesh, Λ, Φ, Φd, inds_l2gd)` (KLDD.jl:850-883) instead and never forms Ψ.

    ξ is a vector (m,) or a panel Ξ (m, nreal); numpy in gives numpy out, a torch CUDA tensor in gives torch CUDA tensors out
    with no host copy (the call is then asynchronous on the context's stream, ordered with torch's current stream)."""

    def __init__(self, ctx: Context, Λ, Ψ):
        Λ, Ψ = _f64(Λ), np.asfortranarray(Ψ, dtype=np.float64)
        if Ψ.ndim != 2 or Ψ.shape[1] != Λ.size:
            raise ValueError(f"Ψ is {Ψ.shape}, Λ has {Λ.size} entries")
        h = vp()
        check(ctx._L.mi_kl_field_create(ctx._h, i64(Ψ.shape[0]), i64(Λ.size), Λ.ctypes.data_as(f64p), Ψ.ctypes.data_as(f64p),
                                        i64(Ψ.shape[0]), C.byref(h)))
        self.ctx, self._h, self.n, self.m, self.factored = ctx, h, Ψ.shape[0], Λ.size, False

    @classmethod
    def from_dd(cls, ctx: Context, nnode: int, Λ, Φ, Φd, inds_l2gd, index_base: int = 0):
        """`inds_l2gd` is 0-based whatever `index_base`: the base is added to the maps on the way to the C call and passed with
        them, so `index_base=1` only sends the arrays as Julia would hold them (the tests use it to reach the C side's shift)."""
        Λ, Φ = _f64(Λ), np.asfortranarray(Φ, dtype=np.float64)
        blocks = [np.asfortranarray(P, dtype=np.float64) for P in Φd]
        maps = [_i64(l2g) + index_base for l2g in inds_l2gd]
        if len(blocks) != len(maps) or any(P.ndim != 2 or P.shape[0] != l.size for P, l in zip(blocks, maps)):
            raise ValueError("Φd[d] must be n_d x md_d with n_d = len(inds_l2gd[d])")
        n_d, md = _i64([P.shape[0] for P in blocks]), _i64([P.shape[1] for P in blocks])
        if Φ.ndim != 2 or Φ.shape != (int(md.sum()), Λ.size):
            raise ValueError(f"Φ is {Φ.shape}, expected {(int(md.sum()), Λ.size)}")
        inds = _i64(np.concatenate(maps)) if maps else _i64([])
        flat = _f64(np.concatenate([P.reshape(-1, order="F") for P in blocks])) if blocks else _f64([])
        h = vp()
        check(ctx._L.mi_kl_field_create_dd(ctx._h, i64(nnode), i64(Λ.size), Λ.ctypes.data_as(f64p), i64(len(blocks)), n_d.ctypes.data_as(i64p),
                                           md.ctypes.data_as(i64p), inds.ctypes.data_as(i64p), C.c_int(index_base), flat.ctypes.data_as(f64p),
                                           Φ.ctypes.data_as(f64p), i64(Φ.shape[0]), C.byref(h)))
        self = cls.__new__(cls)
        self.ctx, self._h, self.n, self.m, self.factored = ctx, h, int(nnode), Λ.size, True
        return self

    def _run(self, ξ, want_g: bool, want_a: bool):
        ctx, n, m = self.ctx, self.n, self.m
        if _is_torch(ξ):
            import torch
            if ξ.dtype != torch.float64 or not ξ.is_cuda:
                raise TypeError("device latent vectors must be float64 CUDA tensors")
            vec = ξ.dim() == 1
            Ξ = ξ.reshape(m, 1) if vec else ξ
            if Ξ.dim() != 2 or Ξ.shape[0] != m:
                raise ValueError(f"ξ is {tuple(ξ.shape)}, expected ({m},) or ({m}, nreal)")
            Ξt = Ξ.t().contiguous()                                    # row r = realization r: column-major (m, nreal)
            nreal = Ξt.shape[0]
            outs = [torch.empty((nreal, n), dtype=torch.float64, device=ξ.device) if w else None for w in (want_g, want_a)]
            check(ctx._L.mi_ctx_set_pointer_mode(ctx._h, _lib.MI_PTR_DEVICE))
            ctx._order((Ξt, *outs), after=False)
            check(ctx._L.mi_kl_field_set(self._h, i64(nreal), vp(Ξt.data_ptr()), i64(m), *[x for o in outs for x in
                                                                                         (vp(o.data_ptr()) if o is not None else None, i64(n))]))
            ctx._order((Ξt, *outs), after=True)
            return [None if o is None else (o[0] if vec else o.t()) for o in outs]
        Ξ = np.asarray(ξ, dtype=np.float64)
        vec = Ξ.ndim == 1
        if Ξ.ndim not in (1, 2) or Ξ.shape[0] != m:
            raise ValueError(f"ξ is {Ξ.shape}, expected ({m},) or ({m}, nreal)")
        Ξ = np.asfortranarray(Ξ.reshape(m, -1))
        nreal = Ξ.shape[1]
        outs = [np.empty((n, nreal), order="F") if w else None for w in (want_g, want_a)]
        check(ctx._L.mi_ctx_set_pointer_mode(ctx._h, _lib.MI_PTR_HOST))
        check(ctx._L.mi_kl_field_set(self._h, i64(nreal), vp(Ξ.ctypes.data), i64(m), *[x for o in outs for x in
                                                                                      (vp(o.ctypes.data) if o is not None else None, i64(n))]))
        return [None if o is None else (o[:, 0].copy() if vec else o) for o in outs]

    def set(self, ξ):
        """g (n,) or G (n, nreal)"""
        return self._run(ξ, True, False)[0]

    def coefficient(self, ξ):
        """a = exp(g)"""
        return self._run(ξ, False, True)[1]

    def set_and_coefficient(self, ξ):
        """(g, a) from one pass over the modes"""
        return tuple(self._run(ξ, True, True))

    def coords(self, M: Operator, g):
        """`get_kl_coordinates(g, Λ, Ψ, M)` (KLDD.jl:1109-1124); `M`: the mass matrix as `SparseMatrixCSC(ctx, M)`. Dense form only."""
        ctx = self.ctx
        ctx._mode_for(g)
        kg, pg = ctx._ptr(g, self.n)
        if _is_torch(g):
            import torch
            out = torch.empty(self.m, dtype=torch.float64, device=g.device)
            po = vp(out.data_ptr())
        else:
            out = np.empty(self.m)
            po = vp(out.ctypes.data)
        ctx._order((kg, out), after=False)
        check(ctx._L.mi_kl_field_coords(self._h, M._h, pg, po))
        ctx._order((kg, out), after=True)
        return out

    def stats(self):
        """{"bytes_kept", "bytes_per_set"}: what the handle keeps on the device, and what one set of one realization streams"""
        a, b = i64(), i64()
        check(self.ctx._L.mi_kl_field_stats(self._h, C.byref(a), C.byref(b)))
        return {"bytes_kept": int(a.value), "bytes_per_set": int(b.value)}

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            self.ctx._L.mi_kl_field_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class McSampler:
    """`McSampler` / `prepare_mc_sampler` / `draw!` / `set!` (Fem/Samplers.jl:1-87). Fields ξ, g, a = exp(g).

    `rng` is a `numpy.random.Generator` (or anything with its `standard_normal(m)` and `random()`); the calls are, in order:
    at construction `standard_normal(m)` for ξ; per `draw()` one `standard_normal(m)`.
    With `field=None` the field is `fem.set_field` on the host (Ψ is needed then); with a `KLField` only ξ crosses to the
    device and g, a come back as numpy arrays (Ψ may be None)."""

    def __init__(self, Λ, Ψ, rng, field: Optional[KLField] = None):
        self.Λ, self.Ψ, self.rng, self.field = _f64(Λ), Ψ, rng, field
        self.m = self.Λ.size
        if field is None and Ψ is None:
            raise ValueError("either Ψ or a KLField is needed")
        self.n = field.n if field is not None else np.asarray(Ψ).shape[0]
        self._init_latent()
        self._field()

    def _init_latent(self):
        self.ξ = np.asarray(self.rng.standard_normal(self.m), dtype=np.float64)

    def _field(self):
        if self.field is not None:
            self.g, self.a = self.field.set_and_coefficient(self.ξ)
        else:
            from . import fem
            self.g = fem.set_field(self.Λ, self.Ψ, self.ξ)
            with np.errstate(over="ignore", invalid="ignore"):
                self.a = np.exp(self.g)

    def draw(self):
        self.ξ = np.asarray(self.rng.standard_normal(self.m), dtype=np.float64)
        self._field()

    def set(self, ξ):
        self.ξ = np.array(ξ, dtype=np.float64).reshape(self.m)
        self._field()


class McmcSampler(McSampler):
    """`McmcSampler` / `prepare_mcmc_sampler` / `draw!` (Fem/Samplers.jl:93-199): random-walk Metropolis on ξ ~ N(0, σ² I) with
    σ² = 1, proposal χ = ξ + ϑ N(0, I), ϑ² = 2.38² σ² / m; α = exp((‖ξ‖² − ‖χ‖²) / 2 / σ²) when ‖ξ‖² < ‖χ‖², else 1; proposals are
    redrawn while u > α and the accepted χ becomes ξ. `draw()` returns cnt, the proposals made. Fields ξ, χ, g, a, σ2, ϑ2.

    Calls of `rng`, in order: at construction `standard_normal(m)` for ξ, then `standard_normal(m)` for χ; per proposal
    `standard_normal(m)`, then `random()` — so a scripted generator reproduces a chain."""

    def _scale(self):
        return self.m

    def _init_latent(self):
        self.σ2 = 1.0
        self.ξ = np.sqrt(self.σ2) * np.asarray(self.rng.standard_normal(self.m), dtype=np.float64)
        k = self._scale()
        self.ϑ2 = 2.38 ** 2 * self.σ2 / k
        self.χ = self.ξ[:k] + np.sqrt(self.ϑ2) * np.asarray(self.rng.standard_normal(k), dtype=np.float64)

    def _metropolis(self, ξ):
        """the loop of Samplers.jl:167-191 on the coordinates ξ -> (accepted χ, cnt)"""
        sq_norm_of_ξ = float(ξ @ ξ)
        cnt = 0
        while True:
            χ = ξ + np.sqrt(self.ϑ2) * np.asarray(self.rng.standard_normal(ξ.size), dtype=np.float64)
            sq_norm_of_χ = float(χ @ χ)
            cnt += 1
            α = float(np.exp((sq_norm_of_ξ - sq_norm_of_χ) / 2 / self.σ2)) if sq_norm_of_ξ < sq_norm_of_χ else 1.0
            u = float(self.rng.random())
            if not u > α:
                return χ, cnt

    def draw(self) -> int:
        self.χ, cnt = self._metropolis(self.ξ)
        self.ξ = self.χ.copy()
        self._field()
        return cnt


class HybridSampler(McmcSampler):
    """`HybridSampler` / `prepare_hybrid_sampler` (Fem/Samplers.jl:208-274): Metropolis on the first m_mcmc coordinates
    (ϑ² = 2.38² σ² / m_mcmc), plain Monte Carlo on the rest. The reference's `draw!` (Samplers.jl:287-322) cannot run as
    written — it reads `smp.n_mcmc`, a field the struct does not have, and the bare names `m` and `m_mcmc` — so this mirrors its
    evident intent: the Metropolis loop on ξ[:m_mcmc], then fresh N(0, 1) numbers for ξ[m_mcmc:]. `draw()` returns cnt.

    Calls of `rng`, in order: at construction `standard_normal(m_mcmc)` and `standard_normal(m - m_mcmc)` for ξ, then
    `standard_normal(m_mcmc)` for χ; per proposal `standard_normal(m_mcmc)`, then `random()`; after the acceptance one
    `standard_normal(m - m_mcmc)`."""

    def __init__(self, Λ, Ψ, rng, m_mcmc: int, field: Optional[KLField] = None):
        if not 1 <= m_mcmc <= _f64(Λ).size:
            raise ValueError(f"m_mcmc = {m_mcmc}: between 1 and m = {_f64(Λ).size} expected")
        self.m_mcmc = int(m_mcmc)
        super().__init__(Λ, Ψ, rng, field)

    def _scale(self):
        return self.m_mcmc

    def _init_latent(self):
        self.σ2 = 1.0
        head = np.sqrt(self.σ2) * np.asarray(self.rng.standard_normal(self.m_mcmc), dtype=np.float64)
        tail = np.asarray(self.rng.standard_normal(self.m - self.m_mcmc), dtype=np.float64)
        self.ξ = np.concatenate([head, tail])
        self.ϑ2 = 2.38 ** 2 * self.σ2 / self.m_mcmc
        self.χ = head + np.sqrt(self.ϑ2) * np.asarray(self.rng.standard_normal(self.m_mcmc), dtype=np.float64)

    def draw(self) -> int:
        self.χ, cnt = self._metropolis(self.ξ[:self.m_mcmc])
        tail = np.asarray(self.rng.standard_normal(self.m - self.m_mcmc), dtype=np.float64)
        self.ξ = np.concatenate([self.χ, tail])
        self._field()
        return cnt


# ------------------------------------------------------------------ quantization of ξ and the operators it selects
# Examples 12-14, 18, 20 (include/mi355schur.h "vector quantization"; kernels in csrc/vq.hpp; host mirror with the same bits in
# fem.py). Matrices are d x ns / d x P with a sample / a centroid per column; numpy in gives numpy out, torch CUDA tensors in
# give torch CUDA tensors out. A numpy view `A[:d, :]` of a Fortran-ordered array, or a torch view `B[:, :d].t()` of a
# contiguous (ns, ld) tensor, is passed with its leading dimension and without a copy: the padding rows are not touched.
def vq_tiling(d: int, ns: int, P: int):
    """`mi_vq_tiling` -> (point_tile, cent_tile, k_chunk, cent_splits, sum_chunk); a pure host function, no device needed."""
    out = [i64() for _ in range(5)]
    check(_lib.load().mi_vq_tiling(i64(d), i64(ns), i64(P), *[C.byref(o) for o in out]))
    return tuple(int(o.value) for o in out)


def _vq_mat(M, writable: bool = False):
    """(keepalive, void*, rows, cols, ld) of a column-major fp64 matrix; a vector is one column."""
    if _is_torch(M):
        import torch
        if M.dtype != torch.float64 or not M.is_cuda:
            raise TypeError("device matrices must be float64 CUDA tensors")
        if M.dim() == 1:
            M = M.reshape(-1, 1)
        r, c = M.shape
        if not ((r == 1 or M.stride(0) == 1) and (c == 1 or M.stride(1) >= r)):
            if writable:
                raise ValueError("an output matrix must be column-major (stride 1 along its rows)")
            M = M.t().contiguous().t()
        return M, vp(M.data_ptr()), r, c, (M.stride(1) if c > 1 else r)
    A = np.asarray(M) if writable else np.asarray(M, dtype=np.float64)
    if A.ndim == 1:
        A = A.reshape(-1, 1)
    r, c = A.shape
    ok = (A.dtype == np.float64 and (r == 1 or A.strides[0] == 8) and (c == 1 or (A.strides[1] >= 8 * r and A.strides[1] % 8 == 0))
          and (A.flags.writeable or not writable))
    if not ok:
        if writable:
            raise ValueError("an output matrix must be a writeable column-major float64 array")
        A = np.asfortranarray(A, dtype=np.float64)
    return A, vp(A.ctypes.data), r, c, (A.strides[1] // 8 if c > 1 else r)


def _vq_out(like, n: int, dtype):
    if _is_torch(like):
        import torch
        t = torch.empty(n, dtype=torch.int64 if dtype == np.int64 else torch.float64, device=like.device)
        return t, vp(t.data_ptr())
    a = np.empty(n, dtype=dtype)
    return a, vp(a.ctypes.data)


def vq_assign(ctx: Context, X, C_, want_assign: bool = True, want_dist2: bool = True, want_objv: bool = True):
    """`mi_vq_assign`: (assign, dist2, objv) — the nearest centroid (0-based) and its squared distance for every column of X,
    and Σ dist2 in the chunked order; an output that is not wanted is None."""
    ctx._mode_for(X, C_)
    kx, px, d, ns, ldx = _vq_mat(X)
    kc, pc, dc, P, ldc = _vq_mat(C_)
    if dc != d:
        raise ValueError(f"X has {d} rows, C has {dc}")
    a, pa = _vq_out(kx, ns, np.int64) if want_assign else (None, None)
    c, pd = _vq_out(kx, ns, np.float64) if want_dist2 else (None, None)
    objv = C.c_double(0.0)
    ctx._order((kx, kc, a, c), after=False)
    check(ctx._L.mi_vq_assign(ctx._h, i64(d), i64(ns), px, i64(ldx), i64(P), pc, i64(ldc), pa, pd, C.byref(objv) if want_objv else None))
    ctx._order((kx, kc, a, c), after=True)
    return a, c, (float(objv.value) if want_objv else None)


def vq_update(ctx: Context, X, assign, C_):
    """`mi_vq_update`: C_ (d x P, column-major, writeable) is updated in place for the assignments; returns (C_, counts)."""
    ctx._mode_for(X, assign, C_)
    kx, px, d, ns, ldx = _vq_mat(X)
    kc, pc, dc, P, ldc = _vq_mat(C_, writable=True)
    if _is_torch(assign):
        ka = assign.contiguous()
        pa = vp(ka.data_ptr())
    else:
        ka = _i64(assign)
        pa = vp(ka.ctypes.data)
    n, pn = _vq_out(kx, P, np.int64)
    ctx._order((kx, kc, ka, n), after=False)
    check(ctx._L.mi_vq_update(ctx._h, i64(d), i64(ns), px, i64(ldx), i64(P), pa, pc, i64(ldc), pn))
    ctx._order((kx, kc, ka, n), after=True)
    return kc, n


def kmpp_seed(ctx: Context, X, P: int, u):
    """`mi_vq_seed`: k-means++ on P uniforms u[j] in [0, 1) -> (picked, C); MiError(MI_ERR_BAD_ARG) with fewer distinct points
    than centres."""
    ctx._mode_for(X, u)
    kx, px, d, ns, ldx = _vq_mat(X)
    ku, pu, nu, _, _ = _vq_mat(u)
    if nu < P:
        raise ValueError(f"{nu} uniforms for {P} centres")
    picked, pp = _vq_out(kx, P, np.int64)
    if _is_torch(kx):
        import torch
        Cn = torch.empty((P, d), dtype=torch.float64, device=kx.device).t()
        pc = vp(Cn.data_ptr())
    else:
        Cn = np.empty((d, P), order="F")
        pc = vp(Cn.ctypes.data)
    ctx._order((kx, ku, picked, Cn), after=False)
    check(ctx._L.mi_vq_seed(ctx._h, i64(d), i64(ns), px, i64(ldx), i64(P), pu, pp, pc, i64(d)))
    ctx._order((kx, ku, picked, Cn), after=True)
    return picked, Cn


class KmeansResult:
    """The fields of Clustering.jl's `KmeansResult` that the reference reads (`res.centers`, `res.assignments`, `res.costs`:
    Ex12F:58), with 0-based assignments."""

    def __init__(self, centers, assignments, costs, counts, totalcost, iterations, converged):
        self.centers, self.assignments, self.costs, self.counts = centers, assignments, costs, counts
        self.totalcost, self.iterations, self.converged = totalcost, iterations, converged


def kmeans(ctx: Context, X, P: int, init="kmpp", rng=None, tol: float = 1e-8, maxiter: int = 1000) -> KmeansResult:
    """`kmeans(X, P, tol=1e-8, maxiter=1_000)` (Ex20F:63; Ex12F:40; Ex13F:143) on the device (`mi_vq_kmeans`). `init`: "kmpp"
    (k-means++ on P uniforms drawn from `rng`, a numpy Generator; Clustering.jl's default), a d x P matrix of centres, or P
    sample indices. An empty cluster keeps its centre (Clustering.jl repicks it at random)."""
    torch_in = _is_torch(X)
    kx, px, d, ns, ldx = _vq_mat(X)
    if isinstance(init, str):
        if init != "kmpp":
            raise ValueError(f"unknown init {init!r}")
        u = (rng if rng is not None else np.random.default_rng()).random(P)
        if torch_in:
            import torch
            u = torch.as_tensor(u, device=kx.device)
        _, C0 = kmpp_seed(ctx, kx, P, u)
    else:
        init = init if _is_torch(init) else np.asarray(init)
        if init.ndim == 1:
            C0 = kx[:, init] if not torch_in else kx[:, init.long() if _is_torch(init) else list(init)]
        else:
            C0 = init
    if torch_in:
        import torch
        Cn = torch.as_tensor(C0, dtype=torch.float64, device=kx.device).t().contiguous().clone().t()
    else:
        Cn = np.array(C0, dtype=np.float64, order="F")
    if tuple(Cn.shape) != (d, P):
        raise ValueError(f"initial centres are {tuple(Cn.shape)}, expected {(d, P)}")
    ctx._mode_for(kx, Cn)
    kc, pc, _, _, ldc = _vq_mat(Cn, writable=True)
    a, pa = _vq_out(kx, ns, np.int64)
    n, pn = _vq_out(kx, P, np.int64)
    c, pd = _vq_out(kx, ns, np.float64)
    objv, it, conv = C.c_double(0.0), i64(0), C.c_int(0)
    ctx._order((kx, kc, a, n, c), after=False)
    check(ctx._L.mi_vq_kmeans(ctx._h, i64(d), i64(ns), px, i64(ldx), i64(P), pc, i64(ldc), C.c_double(tol), i64(maxiter), pa, pn, pd,
                              C.byref(objv), C.byref(it), C.byref(conv)))
    ctx._order((kx, kc, a, n, c), after=True)
    return KmeansResult(kc, a, c, n, float(objv.value), int(it.value), bool(conv.value))


def find_precond(ctx: Context, x, hXt) -> int:
    """`find_precond(x, hXt)` (Ex20F:39-54): the nearest centroid of x, 0-based; the centroids (nKL_trunc x P) are zero-padded
    to length(x) on the host, as the reference does. Host arrays."""
    x, hXt = _f64(x).ravel(), np.asarray(hXt, dtype=np.float64)
    if hXt.ndim != 2 or hXt.shape[0] > x.size:
        raise ValueError(f"hXt is {hXt.shape} for an x of {x.size} entries")
    padded = np.zeros((x.size, hXt.shape[1]), order="F")
    padded[:hXt.shape[0]] = hXt
    return int(vq_assign(ctx, x.reshape(-1, 1), padded, want_dist2=False, want_objv=False)[0][0])


def get_distortion(ctx: Context, X, hXt) -> float:
    """`get_distortion(X, hXt)` (Ex13F:53-69): objv / ns."""
    objv = vq_assign(ctx, X, hXt, want_assign=False, want_dist2=False)[2]
    return objv / int(X.shape[1])


def get_quantizer(ctx: Context, n: int, P: int, Λ, distance: str = "L2-full", rng=None):
    """`get_quantizer(n, P, Λ; distance)` (Ex12F:29-59): n draws of ξ ~ N(0, I), k-means on the data scaled for `distance`
    ("L2-full" / "L2", "L2-10%", "cdf-full", "cdf": fem.scale_data), the centres scaled back. Returns (X, centers, assignments,
    costs) with X the unscaled draws. The reference seeds Julia's generator; here `rng` (a numpy Generator) draws both the
    samples and the k-means++ uniforms."""
    from . import fem
    rng = rng if rng is not None else np.random.default_rng()
    Λ = _f64(Λ)
    X = rng.standard_normal((Λ.size, n))
    res = kmeans(ctx, fem.scale_data(X, Λ, distance), P, init="kmpp", rng=rng)
    return X, fem.unscale_centers(res.centers, Λ, distance), res.assignments, res.costs


class InterpolatingPreconditioner(Operator):
    """`InterpolatingPreconditioner(coefficients, Πs)` (Ex14F:73-113): `Π \\ r` = Σ_i c_i (Πs[i] \\ r), on the device
    (`mi_op_combine`), usable as the `M` of pcg and its relatives. 1 to 16 operators of one context and one size. This
    object keeps references to them, and the library counts them: `close()` of a child raises MiError until every
    combination that holds it is closed. A child may be refreshed under a live combination (`set_values`, `set_correction`,
    `set_coupling`, ...): the next solve uses its new state. A non-finite coefficient — what `fem.shepard_coefficients`
    gives at zero distance — raises ValueError."""

    def __init__(self, ctx: Context, coefficients, Πs: Sequence[Operator]):
        coef = self._coef(coefficients)
        Πs = list(Πs)
        if coef.size != len(Πs):
            raise ValueError(f"{coef.size} coefficients for {len(Πs)} operators")
        hs = (vp * max(len(Πs), 1))(*[p._h for p in Πs])
        h = vp()
        check(ctx._L.mi_op_combine(ctx._h, i64(len(Πs)), hs, coef.ctypes.data_as(f64p), C.byref(h)))
        super().__init__(ctx, h, keep=tuple(Πs))
        self.coefficients, self.Πs = coef, Πs

    @staticmethod
    def _coef(coefficients):
        coef = _f64(coefficients).ravel()
        if not np.all(np.isfinite(coef)):
            raise ValueError("a coefficient is not finite (Shepard weights at zero distance?)")
        return coef

    def set_coefficients(self, coefficients) -> None:
        """New coefficients into the same device array (`mi_op_combine_set_coefficients`); solve graphs stay valid."""
        coef = self._coef(coefficients)
        if coef.size != len(self.Πs):
            raise ValueError(f"{coef.size} coefficients for {len(self.Πs)} operators")
        check(self.ctx._L.mi_op_combine_set_coefficients(self._h, coef.ctypes.data_as(f64p)))
        self.coefficients = coef

    def close(self) -> None:
        super().close()                 # before the children it borrows
        self._keep, self.Πs = (), []


def get_centroidal_preconds(ctx: Context, centroids, field: KLField, assemble: Callable, A0, **amg_kw):
    """`get_centroidal_preconds(centroids, Λ, Ψ)` (Ex12F:85-113): one constant AMG preconditioner per centroid. For column p,
    a = field.coefficient(ξ_p) (`set!` + `exp.(g)`; a centroid with fewer rows than the field has modes is zero-padded, as
    Ex20F:100-101 does), A_p = assemble(a) — a scipy sparse matrix on the pattern of A0, or its CSR values, e.g.
    `lambda a: FullAssemblyPlan(ctx, plan).run(a)[0]` for an assembly that stays on the device — and
    `AMGPreconditioner(ctx, A0, device_setup=True)` + `.set_values(A_p)`: the aggregates are those of A0 for every centroid."""
    centroids = np.asarray(centroids, dtype=np.float64)
    Π = []
    for p in range(centroids.shape[1]):
        ξ = np.zeros(field.m)
        ξ[:centroids.shape[0]] = centroids[:, p]
        # the host set-up (the aggregates) runs once, for the first one
        M = AMGPreconditioner(ctx, A0, device_setup=True, **(amg_kw if not Π else dict(aggregates=Π[0].aggregates)))
        M.set_values(assemble(field.coefficient(ξ)))
        Π.append(M)
    return Π


# ------------------------------------------------------------------ P hierarchies on one plan
AMG_BANK_MAX_TERMS = 16


def amg_bank_member_bytes(H) -> int:
    """`bytes_per_member` of `mi_amg_bank_stats` for the level matrices `H.A`, `H.P` of a `fem.AmgHierarchy` on the structural
    patterns (`fem.amg_refresh(aggregates, A)`, `AMGBank.device_hierarchy(p)`): 8 (Σ_l nnz(A_l) + 2 Σ_{l<L-1} nnz(P_l) +
    Σ_{l<L-1} n_l + n_c² + 2 (L - 1)) plus 8 bytes for every array of an odd count of doubles."""
    L = len(H.A)
    counts = [int(a.indices.size) for a in H.A]
    counts += [int(p.indices.size) for p in H.P] * 2
    counts += [int(a.shape[0]) for a in H.A[:L - 1]]
    counts.append(int(H.A[-1].shape[0]) ** 2)
    return 8 * (sum(c + (c & 1) for c in counts) + 2 * (L - 1))


def _csr_values(v):
    if sp.issparse(v):
        v = sp.csr_matrix(v)
        v.sum_duplicates()
        v.sort_indices()
        v = _f64(v.data)
    return v


class AMGBank:
    """`capacity` smoothed-aggregation hierarchies on the pattern and the frozen aggregates of `A0`, sharing ONE plan, one set
    of index arrays and one set-up engine on the device (`mi_amg_bank_create`): the constant preconditioners of the
    quantization studies (`get_centroidal_preconds`, Ex12F:85-113) at a P where separate `AMGPreconditioner` objects do not
    fit. A member is numbers only. `aggregates=[agg_0, …]` (0-based, one array per smoothed level) come from
    `fem.prepare_amg_precond(A0, **amg_kw)` unless given. The bank is not an operator: solve and apply with `.view()`.
    Members are 0-based."""

    def __init__(self, ctx: Context, A0, capacity: int, index_base: int = 0, aggregates=None, **amg_kw):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity = {capacity}: a bank holds at least 1 member")
        if index_base not in (0, 1):
            raise ValueError(f"index_base = {index_base} (0 or 1)")
        if not (sp.issparse(A0) or isinstance(A0, np.ndarray)):
            raise TypeError("AMGBank takes the matrix whose pattern every member shares")
        A = sp.csr_matrix(A0)
        A.sum_duplicates()
        A.sort_indices()
        if A.shape[0] != A.shape[1]:
            raise ValueError("square matrix expected")
        if aggregates is not None:
            if amg_kw:
                raise TypeError(f"set-up options {sorted(amg_kw)} with aggregates that are already chosen")
            agg0 = [_i64(a).ravel() for a in aggregates]
            sizes = [A.shape[0]] + [int(a.max()) + 1 if a.size else 0 for a in agg0]
        else:
            from . import fem
            H = fem.prepare_amg_precond(A, **amg_kw)
            agg0, sizes = [_i64(a).ravel() for a in H.agg], list(H.sizes)
        aggs = [a + index_base for a in agg0]
        n_l = _i64(sizes)
        ptr, idx = _i64(A.indptr) + index_base, _i64(A.indices) + index_base
        h = vp()
        check(ctx._L.mi_amg_bank_create(ctx._h, i64(A.shape[0]), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), i64(len(sizes)),
                                        n_l.ctypes.data_as(i64p), _ptrs(aggs, i64p) if aggs else None, i64(capacity),
                                        C.c_int(index_base), C.byref(h)))
        self.ctx, self._h = ctx, h
        self.n, self.nnz, self.capacity, self.n_levels = int(A.shape[0]), int(A.indices.size), capacity, len(sizes)
        self.aggregates = list(agg0)
        self._views = []

    def _member(self, p) -> int:
        q = int(p)
        if q != p or not 0 <= q < self.capacity:
            raise IndexError(f"member {p} outside 0 .. {self.capacity - 1}")
        return q

    def set_values(self, p: int, A_or_nzval) -> None:
        """The hierarchy of member `p` from a matrix on the pattern of `A0`: a scipy sparse matrix, or its CSR values as a numpy
        array or a torch CUDA tensor (`mi_amg_bank_set_values`). Synchronous. MiError(MI_ERR_SINGULAR) leaves the member as
        it was (unset, if it never was set)."""
        p = self._member(p)
        v = _csr_values(A_or_nzval)
        count = v.numel() if _is_torch(v) else np.size(v)
        if count != self.nnz:
            raise ValueError(f"{count} values for the {self.nnz} stored entries of the bank's pattern")
        self.ctx._mode_for(v)
        k, ptr = self.ctx._ptr(v, self.nnz)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_amg_bank_set_values(self._h, i64(p), ptr))   # synchronous

    def set_values_batch(self, members, batch: "CsrBatch", slots, strict: bool = True) -> np.ndarray:
        """The hierarchies of k <= 16 members in one sequence of launches (`mi_amg_bank_set_values_batch`): member
        `members[t]` from the values in slot `slots[t]` of a `CsrBatch` on the bank's pattern, read on the device where they
        lie. A member carries the bits of `set_values(members[t], values)`. Synchronous. Returns a boolean array of per-term
        success; a failed term leaves its member as it was, the healthy terms are committed. With `strict` a failed term
        raises MiError(MI_ERR_SINGULAR) after that commit (the array is the exception's `.ok`)."""
        mem, sl = _i64(members).ravel(), _i64(slots).ravel()
        if mem.size != sl.size:
            raise ValueError(f"{mem.size} members for {sl.size} slots")
        status = (C.c_int * max(int(mem.size), 1))()
        check(self.ctx._L.mi_amg_bank_set_values_batch(self._h, i64(int(mem.size)), mem.ctypes.data_as(i64p), getattr(batch, "_h", None),
                                                       sl.ctypes.data_as(i64p), status))
        ok = np.array([status[t] == _lib.MI_OK for t in range(mem.size)], dtype=bool)
        if strict and not ok.all():
            try:
                check(_lib.MI_ERR_SINGULAR)   # the library's message names the failed terms and their reasons
            except MiError as e:
                e.ok = ok
                raise
        return ok

    def view(self, max_terms: int = 1) -> "AMGBankView":
        """An operator on this bank for up to `max_terms` (1 .. 16) members at a time; it selects member 0 at first."""
        v = AMGBankView(self, max_terms)
        self._views.append(v)
        return v

    def stats(self) -> dict:
        """dict(capacity, members_set, bytes_shared, bytes_per_member, views) (`mi_amg_bank_stats`)"""
        a, b, c, d, e = i64(), i64(), i64(), i64(), i64()
        check(self.ctx._L.mi_amg_bank_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return dict(capacity=int(a.value), members_set=int(b.value), bytes_shared=int(c.value), bytes_per_member=int(d.value),
                    views=int(e.value))

    def device_hierarchy(self, p: int):
        """Member `p` as the device holds it, a `fem.AmgHierarchy` (`mi_amg_bank_level_sizes`, `mi_amg_bank_level_get`,
        `mi_amg_bank_coarse_inverse`)."""
        from . import fem
        p = self._member(p)
        L = self.ctx._L
        As, Ps, om, owd = [], [], [], []
        for l in range(self.n_levels):
            n, m, an, pn = i64(), i64(), i64(), i64()
            check(L.mi_amg_bank_level_sizes(self._h, i64(l), C.byref(n), C.byref(m), C.byref(an), C.byref(pn)))
            n, m, an, pn = int(n.value), int(m.value), int(an.value), int(pn.value)
            ap, ai, av = np.zeros(n + 1, dtype=np.int64), np.zeros(an, dtype=np.int64), np.zeros(an)
            pp, pi, pv = np.zeros(n + 1, dtype=np.int64), np.zeros(pn, dtype=np.int64), np.zeros(pn)
            w, wd = C.c_double(0.0), np.zeros(n)
            check(L.mi_amg_bank_level_get(self._h, i64(p), i64(l), ap.ctypes.data_as(i64p), ai.ctypes.data_as(i64p),
                                          av.ctypes.data_as(f64p), pp.ctypes.data_as(i64p), pi.ctypes.data_as(i64p),
                                          pv.ctypes.data_as(f64p), C.byref(w), wd.ctypes.data_as(f64p)))
            As.append(sp.csr_matrix((av, ai, ap), shape=(n, n)))
            if l < self.n_levels - 1:
                Ps.append(sp.csr_matrix((pv, pi, pp), shape=(n, m)))
                om.append(float(w.value)); owd.append(wd)
        nc = As[-1].shape[0]
        inv = np.zeros((nc, nc), order="F")
        check(L.mi_amg_bank_coarse_inverse(self._h, i64(p), inv.ctypes.data_as(f64p)))
        nnz = [a.indices.size for a in As]
        return fem.AmgHierarchy(As, Ps, om, owd, inv, [a.shape[0] for a in As], float(sum(nnz)) / float(nnz[0]), self.aggregates)

    def close(self) -> None:
        """`mi_op_destroy` of the bank, after its views that are still open (the library refuses a bank under a live view)."""
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            for v in list(self._views):
                v.close()
            check(self.ctx._L.mi_op_destroy(self._h))
        self._h, self._views = None, []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AMGBankView(Operator):
    """`bank.view(max_terms)`: `Π \\ r` = Σ_i c_i (Π_{m_i} \\ r) over members of an `AMGBank` (`mi_amg_bank_view`), usable as the
    `M` of pcg and its relatives, as a child of `InterpolatingPreconditioner` and through `.ldiv(r)`. `.select(p)` is the
    `Πs[find_precond(ξ, hXt)]` of Example12, `.combine(members, coefficients)` the `InterpolatingPreconditioner` of
    Example14 — both rewrite small device arrays, so the solve graphs captured with the view serve every selection."""

    def __init__(self, bank: AMGBank, max_terms: int = 1):
        kmax = int(max_terms)
        if kmax != max_terms or not 1 <= kmax <= AMG_BANK_MAX_TERMS:
            raise ValueError(f"max_terms = {max_terms} (1 <= max_terms <= {AMG_BANK_MAX_TERMS})")
        if not getattr(bank, "_h", None):
            raise ValueError("the bank is closed")
        h = vp()
        check(bank.ctx._L.mi_amg_bank_view(bank._h, i64(kmax), C.byref(h)))
        super().__init__(bank.ctx, h, keep=(bank,))
        self.bank, self.max_terms = bank, kmax
        self.members, self.coefficients = np.zeros(1, dtype=np.int64), np.ones(1)

    def select(self, p: int) -> None:
        """One member, coefficient 1."""
        self.combine([p], [1.0])

    def combine(self, members, coefficients) -> None:
        """k members (1 <= k <= max_terms, each set before; one may appear twice) and k finite coefficients
        (`mi_amg_bank_select`)."""
        mem = [self.bank._member(p) for p in np.asarray(members).ravel().tolist()]
        coef = _f64(coefficients).ravel()
        if not 1 <= len(mem) <= self.max_terms:
            raise ValueError(f"k = {len(mem)} members (1 <= k <= max_terms = {self.max_terms})")
        if coef.size != len(mem):
            raise ValueError(f"{coef.size} coefficients for {len(mem)} members")
        if not np.all(np.isfinite(coef)):
            raise ValueError("a coefficient is not finite (Shepard weights at zero distance?)")
        mem = _i64(mem)
        check(self.ctx._L.mi_amg_bank_select(self._h, i64(mem.size), mem.ctypes.data_as(i64p), coef.ctypes.data_as(f64p)))
        self.members, self.coefficients = mem, coef

    def close(self) -> None:
        super().close()
        bank = getattr(self, "bank", None)
        if bank is not None and self in bank._views:
            bank._views.remove(self)
        self._keep = ()


def get_centroidal_bank(ctx: Context, centroids, field: KLField, assemble, A0, batch: int = 0, **amg_kw) -> AMGBank:
    """`get_centroidal_preconds` on a bank: member p is the constant AMG preconditioner of centroid p (column p of
    `centroids`, zero-padded to the field's modes), `assemble(a)` as there. One plan, one set of index arrays, P slots of
    numbers: `bank.view().select(find_precond(ctx, ξ, hXt))` is the `Πs[p]` of Example12:106.

    `batch = k` (1 .. 16): `assemble` is a `FullAssemblyPlan` on the pattern of `A0`; the centroids' matrices are assembled k
    at a time into a `CsrBatch` (`update_batch`) and k members are refreshed per call (`AMGBank.set_values_batch`; the last
    call is short when k does not divide P). The members carry the bits of the default path on the same matrices."""
    centroids = np.asarray(centroids, dtype=np.float64)
    P = centroids.shape[1]
    k = int(batch)
    if k != batch or not 0 <= k <= AMG_BANK_MAX_TERMS:
        raise ValueError(f"batch = {batch} (0: one member per call; 1 <= batch <= {AMG_BANK_MAX_TERMS})")
    if k and not hasattr(assemble, "update_batch"):
        raise TypeError("with batch > 0, `assemble` is the FullAssemblyPlan whose update_batch fills the slots")

    def coefficient(p):
        ξ = np.zeros(field.m)
        ξ[:centroids.shape[0]] = centroids[:, p]
        return field.coefficient(ξ)

    bank = AMGBank(ctx, A0, P, **amg_kw)
    if not k:
        for p in range(P):
            bank.set_values(p, assemble(coefficient(p)))
        return bank
    slab = CsrBatch(ctx, A0, k)
    try:
        for p0 in range(0, P, k):
            members = np.arange(p0, min(p0 + k, P))
            for s, p in enumerate(members):
                assemble.update_batch(coefficient(p), slab, s)
            bank.set_values_batch(members, slab, np.arange(members.size))
    except Exception:
        bank.close()
        raise
    finally:
        slab.close()
    return bank


# ------------------------------------------------------------------ k realizations in one Krylov loop
CSR_BATCH_MAX = 16   # systems of one `pcg_batch` (= AMG_BANK_MAX_TERMS: one term of a bank view each)


def csr_batch_slot_bytes(nnz: int) -> int:
    """`bytes_per_slot` of `mi_csr_batch_stats` for `nnz` stored entries: 8 (nnz + nnz mod 2) (`mi_csr_batch_stride`; no device)."""
    d = i64()
    check(_lib.load().mi_csr_batch_stride(i64(int(nnz)), C.byref(d)))
    return 8 * int(d.value)


class CsrBatch:
    """`capacity` sparse matrices on the pattern of `A0`, sharing one set of index arrays and row blocks on the device
    (`mi_csr_batch_create`): the systems A_t of a Monte-Carlo loop over realizations. A slot is numbers only. The batch is
    not an operator: `pcg_batch` solves k of its slots in one Krylov loop. Slots are 0-based."""

    def __init__(self, ctx: Context, A0, capacity: int, index_base: int = 0):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"capacity = {capacity}: a batch holds at least 1 slot")
        if index_base not in (0, 1):
            raise ValueError(f"index_base = {index_base} (0 or 1)")
        if not (sp.issparse(A0) or isinstance(A0, np.ndarray)):
            raise TypeError("CsrBatch takes the matrix whose pattern every slot shares")
        A = sp.csr_matrix(A0)
        A.sum_duplicates()
        A.sort_indices()
        if A.shape[0] != A.shape[1]:
            raise ValueError("square matrix expected")
        ptr, idx = _i64(A.indptr) + index_base, _i64(A.indices) + index_base
        h = vp()
        check(ctx._L.mi_csr_batch_create(ctx._h, i64(A.shape[0]), ptr.ctypes.data_as(i64p), idx.ctypes.data_as(i64p), i64(capacity),
                                         C.c_int(index_base), C.byref(h)))
        self.ctx, self._h = ctx, h
        self.n, self.nnz, self.capacity = int(A.shape[0]), int(A.indices.size), capacity

    def _slot(self, s) -> int:
        q = int(s)
        if q != s or not 0 <= q < self.capacity:
            raise IndexError(f"slot {s} outside 0 .. {self.capacity - 1}")
        return q

    def set_values(self, slot: int, A_or_nzval) -> None:
        """Slot `slot` from a matrix on the pattern of `A0`: a scipy sparse matrix, or its CSR values as a numpy array or a
        torch CUDA tensor (`mi_csr_batch_set_values`; a tensor is copied asynchronously on the context's stream)."""
        slot = self._slot(slot)
        v = _csr_values(A_or_nzval)
        count = v.numel() if _is_torch(v) else np.size(v)
        if count != self.nnz:
            raise ValueError(f"{count} values for the {self.nnz} stored entries of the batch's pattern")
        self.ctx._mode_for(v)
        k, ptr = self.ctx._ptr(v, self.nnz)
        self.ctx._order((k,), after=False)
        check(self.ctx._L.mi_csr_batch_set_values(self._h, i64(slot), ptr))
        self.ctx._record(k)

    def get_values(self, slot: int):
        """The CSR values of slot `slot` as the device holds them, a numpy array (`mi_csr_batch_get_values`)."""
        slot = self._slot(slot)
        out = np.empty(self.nnz)
        self.ctx._mode_for(out)
        check(self.ctx._L.mi_csr_batch_get_values(self._h, i64(slot), vp(out.ctypes.data)))
        return out

    def stats(self) -> dict:
        """dict(capacity, slots_set, bytes_shared, bytes_per_slot) (`mi_csr_batch_stats`)"""
        a, b, c, d = i64(), i64(), i64(), i64()
        check(self.ctx._L.mi_csr_batch_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(capacity=int(a.value), slots_set=int(b.value), bytes_shared=int(c.value), bytes_per_slot=int(d.value))

    def close(self) -> None:
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            check(self.ctx._L.mi_op_destroy(self._h))
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _batch_matrix(ctx: Context, V, n: int, k: int, what: str, copy: bool):
    """(keepalive, void*, ld) of an n x k column-major block: a torch CUDA tensor with unit row stride (used in place, its
    column stride is the leading dimension) or a numpy array (a Fortran-ordered view with a column stride >= n is used as it
    is unless `copy`)."""
    if _is_torch(V):
        import torch
        if V.dtype != torch.float64 or not V.is_cuda or V.dim() != 2 or tuple(V.shape) != (n, k) or V.stride(0) != 1 or (k > 1 and V.stride(1) < n):
            raise TypeError(f"{what} must be an {n} x {k} column-major float64 CUDA tensor (e.g. torch.empty(k, n).T)")
        return V, vp(V.data_ptr()), int(V.stride(1)) if k > 1 else n
    a = np.asarray(V)
    if a.ndim == 1 and k == 1:
        a = a.reshape(n, 1)
    if a.shape != (n, k):
        raise ValueError(f"{what} must be {n} x {k}, got {a.shape}")
    direct = (not copy and a.dtype == np.float64 and a.strides[0] == 8 and (k == 1 or (a.strides[1] % 8 == 0 and a.strides[1] >= 8 * n)))
    if not direct:
        a = np.array(a, dtype=np.float64, order="F", copy=True)
    return a, vp(a.ctypes.data), (a.strides[1] // 8 if k > 1 else n)


def pcg_batch(A_batch: CsrBatch, slots, B, X0, M_view: Optional["AMGBankView"], members=None, maxit: int = 0, eps: float = EPS,
              ldres: Optional[int] = None):
    """k solves in one Krylov loop (`mi_pcg_batch`): for t < k, `pcg(A[slots[t]], B[:, t], X0[:, t], Π[members[t]])` with the
    matrices of a `CsrBatch` and the members of the bank under `M_view` (`M_view=None`: cg). Returns `(X, its, [res_norm_t])`;
    x, it and res_norm of system t carry the bits of its separate solve with `M_view.select(members[t])`. numpy in -> a new
    Fortran-ordered X out; torch CUDA tensors (column-major) -> X0 is mutated in place. `ldres`: the capacity of every residual
    history (default: as the single solvers); BoundsError carries `.X` and `.its` when a system needed more."""
    ctx, n = A_batch.ctx, A_batch.n
    sl = _i64(slots).ravel()
    k = int(sl.size)
    if M_view is not None:
        if members is None:
            raise ValueError("members is required with a preconditioner view")
        mem = _i64(members).ravel()
        if mem.size != k:
            raise ValueError(f"{mem.size} members for {k} slots")
        pm = mem.ctypes.data_as(i64p)
    else:
        mem, pm = None, None
    ctx._mode_for(B, X0)
    kB, pB, ldb = _batch_matrix(ctx, B, n, k, "B", copy=False)
    kX, pX, ldx = _batch_matrix(ctx, X0, n, k, "X0", copy=not _is_torch(X0))
    cap = int(ldres) if ldres is not None else int(min(maxit if maxit else n, n)) + 1
    res = np.empty((max(cap, 1), max(k, 1)), order="F")
    its = np.zeros(max(k, 1), dtype=np.int64)
    ctx._order((kB, kX), after=False)
    rc = ctx._L.mi_pcg_batch(A_batch._h, i64(k), sl.ctypes.data_as(i64p), getattr(M_view, "_h", None), pm, pB, i64(ldb), pX, i64(ldx),
                             i64(maxit), C.c_double(eps), res.ctypes.data_as(f64p), i64(cap), its.ctypes.data_as(i64p))
    ctx._order((kB, kX), after=True)
    its = its[:k]
    try:
        check(rc)
    except BoundsError as e:
        e.X, e.its = kX, its.copy()
        raise
    return kX, its.copy(), [res[:int(its[t]), t].copy() for t in range(k)]
