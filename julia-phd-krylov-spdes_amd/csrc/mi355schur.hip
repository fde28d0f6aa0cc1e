// extern "C" surface of libmi355schur (see include/mi355schur.h for the contract of every symbol).
#include <dlfcn.h>

#include <thread>
#include <tuple>

#include "eig_solvers.hpp"
#include "lanczos.hpp"
#include "setup_gj.hpp"
#include "pinv_spectral.hpp"
#include "spd_direct.hpp"
#include "lorasc.hpp"
#include "nn_induced.hpp"
#include "block_jacobi.hpp"
#include "amg.hpp"
#include "amg_setup.hpp"
#include "amg_bank.hpp"
#include "batch_solvers.hpp"
#include "interior_amg.hpp"
#include "kl.hpp"
#include "kl_field.hpp"
#include "vq.hpp"
#include "full_assembly.hpp"

namespace mi {

Rccl &Rccl::get() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    // Prefer an RCCL that is already in the process (e.g. the one torch loaded), else the system one.
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names) {
      r.handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
      if (r.handle) break;
    }
    if (r.handle) {
      r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.handle, "ncclGetUniqueId");
      r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.handle, "ncclCommInitRank");
      r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.handle, "ncclCommDestroy");
      r.AllReduce = (decltype(r.AllReduce))dlsym(r.handle, "ncclAllReduce");
      r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.handle, "ncclGetErrorString");
    }
  }
  if (!r.handle || !r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.GetErrorString)
    raise(MI_ERR_COMM, "librccl could not be loaded: %s", dlerror() ? dlerror() : "missing symbols");
  return r;
}

// Input vector in the caller's pointer mode -> device pointer valid on ctx->stream.
struct In {
  const double *dev;
  In(mi_ctx_s *c, const double *p, size_t n, DevBuf<double> &stage) {
    if (c->ptr_mode == MI_PTR_DEVICE || n == 0) { dev = p; return; }
    stage.ensure(n);
    MI_HIP(hipMemcpyAsync(stage.p, p, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    dev = stage.p;
  }
};
// In/out vector: staged on entry, copied back by finish().
struct InOut {
  mi_ctx_s *c; double *user; double *dev; size_t n; bool staged;
  InOut(mi_ctx_s *c_, double *p, size_t n_, DevBuf<double> &stage, bool read) : c(c_), user(p), n(n_) {
    staged = c->ptr_mode != MI_PTR_DEVICE && n > 0;
    if (!staged) { dev = p; return; }
    stage.ensure(n);
    dev = stage.p;
    if (read) MI_HIP(hipMemcpyAsync(dev, p, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  void finish() {
    if (staged) {
      MI_HIP(hipMemcpyAsync(user, dev, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      MI_HIP(hipStreamSynchronize(c->stream));
    }
  }
};

static double reduce_to_host(mi_ctx_s *c, int g, int take_sqrt) {
  c->scalar.ensure(1);
  hipLaunchKernelGGL(k_finish_sum, dim3(1), dim3(NT), 0, c->stream, c->partials.p, g, c->scalar.p, take_sqrt);
  MI_HIP(hipGetLastError());
  double out = 0.0;
  MI_HIP(hipMemcpyAsync(&out, c->scalar.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  MI_HIP(hipStreamSynchronize(c->stream));
  return out;
}

// out[i] = Σ_r in[r][i], r ascending (the loopback communicator's reduction)
__global__ __launch_bounds__(NT) void k_loop_sum(size_t n, int nr, const double *const *in, double *__restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    double s = in[0][i];
    for (int r = 1; r < nr; ++r) s += in[r][i];
    out[i] = s;
  }
}

void loop_allreduce(LoopGroup &g, int rank, const double *send, double *recv, size_t n, hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cap);
  if (cap != hipStreamCaptureStatusNone) raise(MI_ERR_COMM, "the loopback communicator cannot be captured into a graph");
  MI_HIP(hipStreamSynchronize(s));               // this rank's buffer is complete before it is published
  g.send[rank] = send;
  g.barrier();                                   // every rank has published a complete buffer
  DevBuf<const double *> ptrs;
  ptrs.upload(g.send.data(), g.send.size(), s);
  DevBuf<double> tmp(n);                         // in-place calls (recv == send) must not be overwritten while others read
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((n + NT - 1) / NT, 1024));
  hipLaunchKernelGGL(k_loop_sum, dim3(grid), dim3(NT), 0, s, n, g.n, ptrs.p, tmp.p);
  MI_HIP(hipGetLastError());
  MI_HIP(hipStreamSynchronize(s));               // done reading everyone's buffer
  g.barrier();                                   // nobody overwrites a send buffer before all ranks have read it
  MI_HIP(hipMemcpyAsync(recv, tmp.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  MI_HIP(hipStreamSynchronize(s));
}

// A handle that cannot be applied as it stands (an AMG bank; a view whose selection was never set): refused before any launch
static int refuse_unusable(const char *me, std::initializer_list<mi_op_t> ops) {
  std::string why;
  for (mi_op_t o : ops)
    if (o && o->impl && !o->impl->usable(why)) return fail(MI_ERR_BAD_ARG, "%s: %s", me, why.c_str());
  return MI_OK;
}

static int run_solver(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit,
                      double eps, double *res_norm, int64_t res_cap, int64_t *it, bool want_M, bool want_W) {
  if (!A || !A->impl || !b || !x || !it || res_cap < 0 || (res_cap > 0 && !res_norm) || maxit < 0)
    return fail(MI_ERR_BAD_ARG, "solver: NULL or negative argument");
  if (want_M && (!M || !M->impl)) return fail(MI_ERR_BAD_ARG, "solver: preconditioner handle is NULL");
  if (want_W && (nvec < 0 || (nvec > 0 && !W) || nvec > 1024)) return fail(MI_ERR_BAD_ARG, "solver: bad W / nvec");
  Operator *a = A->impl.get(), *m = want_M ? M->impl.get() : nullptr;
  if (m && (m->n != a->n || m->ctx != a->ctx)) return fail(MI_ERR_BAD_ARG, "solver: A and M differ in size or context");
  if (int rc = refuse_unusable("solver", {A, want_M ? M : nullptr})) return rc;
  mi_ctx_s *c = a->ctx;
  return guarded([&]() -> int {
    c->use();
    const size_t n = (size_t)a->n;
    DevBuf<double> wstage;
    In wi(c, W, want_W ? n * (size_t)nvec : 0, wstage);
    Krylov k(c, a, m, want_W ? (int)nvec : 0);
    if (c->ptr_mode == MI_PTR_DEVICE) return k.solve(b, x, wi.dev, maxit, eps, res_norm, res_cap, it);
    // Host pointers (Julia arrays): b and x0 go through pinned buffers that the solve's entry kernel reads and its
    // exit kernel writes directly — no copy operations on the stream, one wait per solve.
    c->pin_b.ensure(n); c->pin_x.ensure(n);
    std::memcpy(c->pin_b.p, b, n * sizeof(double));
    std::memcpy(c->pin_x.p, x, n * sizeof(double));
    const int rc = k.solve(c->pin_b.p, c->pin_x.p, wi.dev, maxit, eps, res_norm, res_cap, it);  // synchronises before returning
    std::memcpy(x, c->pin_x.p, n * sizeof(double));
    return rc;
  });
}

static int run_eig_solver(EigKind kind, mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec,
                          int64_t spdim, int64_t maxit, double eps, double *res_norm, int64_t res_cap, int64_t *it,
                          double *V_out) {
  const bool want_M = kind == EIGPCG || kind == EIGDEFPCG, want_W = kind == EIGDEFCG || kind == EIGDEFPCG;
  if (!A || !A->impl || !b || !x || !it || res_cap < 0 || (res_cap > 0 && !res_norm) || maxit < 0)
    return fail(MI_ERR_BAD_ARG, "solver: NULL or negative argument");
  if (want_M && (!M || !M->impl)) return fail(MI_ERR_BAD_ARG, "solver: preconditioner handle is NULL");
  if (nvec < 1 || nvec > 512 || spdim > 4096 || (want_W && !W)) return fail(MI_ERR_BAD_ARG, "solver: bad W / nvec / spdim");
  if (spdim < 2 * nvec + 1)
    return fail(MI_ERR_BOUNDS, "spdim = %lld < 2 nvec + 1 = %lld: V[:, nev + 1] can fall outside the search space (BoundsError)",
                (long long)spdim, (long long)(2 * nvec + 1));
  Operator *a = A->impl.get(), *m = want_M ? M->impl.get() : nullptr;
  if (m && (m->n != a->n || m->ctx != a->ctx)) return fail(MI_ERR_BAD_ARG, "solver: A and M differ in size or context");
  if (int rc = refuse_unusable("solver", {A, want_M ? M : nullptr})) return rc;
  mi_ctx_s *c = a->ctx;
  return guarded([&]() -> int {
    c->use();
    const size_t n = (size_t)a->n;
    In bi(c, b, n, c->scratch_a);
    InOut xi(c, x, n, c->scratch_b, true);
    DevBuf<double> wstage, vstage;
    In wi(c, W, want_W ? n * (size_t)nvec : 0, wstage);
    InOut vi(c, V_out, V_out ? n * (size_t)nvec : 0, vstage, false);
    EigKrylov k(c, a, m, kind, (int)nvec, (int)spdim);
    const int rc = k.solve(bi.dev, xi.dev, wi.dev, maxit, eps, res_norm, res_cap, it, V_out ? vi.dev : nullptr);
    xi.finish();
    vi.finish();
    return rc;
  });
}

// initcg / initpcg (initcg.jl:28-75, 106-160): x += W (WtAW \ W'(b - A x)), then cg / pcg from that guess.
static int run_init_solver(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit,
                           double eps, double *res_norm, int64_t res_cap, int64_t *it, bool want_M) {
  if (!A || !A->impl || !b || !x || !it || res_cap < 0 || (res_cap > 0 && !res_norm) || maxit < 0)
    return fail(MI_ERR_BAD_ARG, "solver: NULL or negative argument");
  if (want_M && (!M || !M->impl)) return fail(MI_ERR_BAD_ARG, "solver: preconditioner handle is NULL");
  if (nvec < 1 || !W || nvec > 1024) return fail(MI_ERR_BAD_ARG, "solver: bad W / nvec");
  Operator *a = A->impl.get(), *m = want_M ? M->impl.get() : nullptr;
  if (m && (m->n != a->n || m->ctx != a->ctx)) return fail(MI_ERR_BAD_ARG, "solver: A and M differ in size or context");
  if (int rc = refuse_unusable("solver", {A, want_M ? M : nullptr})) return rc;
  mi_ctx_s *c = a->ctx;
  return guarded([&]() -> int {
    c->use();
    const size_t n = (size_t)a->n;
    In bi(c, b, n, c->scratch_a);
    InOut xi(c, x, n, c->scratch_b, true);
    DevBuf<double> wstage;
    In wi(c, W, n * (size_t)nvec, wstage);
    {
      Krylov guess(c, a, nullptr, (int)nvec, /*generic=*/true);
      int64_t mx = maxit, cap = 0;
      double e = eps;
      guess.begin(bi.dev, xi.dev, wi.dev, mx, e, cap);   // leaves the deflated guess in the workspace's x
      MI_HIP(hipMemcpyAsync(xi.dev, guess.ws.x, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    Krylov k(c, a, m, 0);
    const int rc = k.solve(bi.dev, xi.dev, nullptr, maxit, eps, res_norm, res_cap, it);
    xi.finish();
    return rc;
  });
}

void peer_allreduce(PeerComm &p, const double *send, double *recv, size_t n, hipStream_t s) { p.allreduce(send, recv, n, s); }
}  // namespace mi

using namespace mi;

extern "C" {

int mi_version(void) { return 400; }  // 0.4.0
const char *mi_last_error(void) { return last_error().c_str(); }

int mi_device_count(int *count) {
  if (!count) return fail(MI_ERR_BAD_ARG, "count is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return MI_OK;
}

int mi_ctx_create(int device, mi_ctx_t *ctx) {
  if (!ctx) return fail(MI_ERR_BAD_ARG, "ctx is NULL");
  *ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(MI_ERR_NO_DEVICE, "no HIP device visible: libmi355schur has no CPU fallback");
  if (device < 0 || device >= n) return fail(MI_ERR_BAD_ARG, "device %d out of range [0,%d)", device, n);
  return guarded([&]() -> int {
    hipDeviceProp_t prop;
    MI_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !std::getenv("MI355_ALLOW_ANY_ARCH"))
      return fail(MI_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    std::unique_ptr<mi_ctx_s> c(new mi_ctx_s);
    c->device = device;
    c->use();
    MI_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    c->chunk = env_int("MI355_CHUNK", 8);
    c->partials.alloc(MAX_PARTS);
    c->scalar.alloc(1);
    *ctx = c.release();
    return MI_OK;
  });
}

int mi_ctx_destroy(mi_ctx_t ctx) {
  if (!ctx) return MI_OK;
  return guarded([&]() -> int {
    ctx->use();
    (void)hipStreamSynchronize(ctx->stream);
    ctx->workspaces.clear();
    if (ctx->comm) (void)Rccl::get().CommDestroy(ctx->comm);
    delete ctx->peer;
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return MI_OK;
  });
}

int mi_ctx_set_pointer_mode(mi_ctx_t ctx, int mode) {
  if (!ctx || (mode != MI_PTR_HOST && mode != MI_PTR_DEVICE)) return fail(MI_ERR_BAD_ARG, "bad ctx or pointer mode");
  ctx->ptr_mode = mode;
  return MI_OK;
}

int mi_ctx_set_stream(mi_ctx_t ctx, void *hip_stream) {
  if (!ctx) return fail(MI_ERR_BAD_ARG, "ctx is NULL");
  return guarded([&]() -> int {
    ctx->use();
    MI_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();  // graphs are tied to the capture stream
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return MI_OK;
  });
}

int mi_ctx_get_stream(mi_ctx_t ctx, void **hip_stream) {
  if (!ctx || !hip_stream) return fail(MI_ERR_BAD_ARG, "NULL argument");
  *hip_stream = (void *)ctx->stream;
  return MI_OK;
}

int mi_ctx_synchronize(mi_ctx_t ctx) {
  if (!ctx) return fail(MI_ERR_BAD_ARG, "ctx is NULL");
  return guarded([&]() -> int { ctx->use(); MI_HIP(hipStreamSynchronize(ctx->stream)); return MI_OK; });
}

int mi_ctx_set_chunk(mi_ctx_t ctx, int iterations_per_graph) {
  if (!ctx || iterations_per_graph < 0 || iterations_per_graph > 4096) return fail(MI_ERR_BAD_ARG, "bad ctx or chunk");
  ctx->chunk = iterations_per_graph;
  return MI_OK;
}

// ---------------------------------------------------------------- multi-GPU
int mi_comm_unique_id(void *id_out) {
  if (!id_out) return fail(MI_ERR_BAD_ARG, "id_out is NULL");
  return guarded([&]() -> int {
    static_assert(sizeof(ncclUniqueId) == MI_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    MI_NCCL(Rccl::get().GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return MI_OK;
  });
}

int mi_ctx_comm_init(mi_ctx_t ctx, const void *id, int rank, int n_ranks) {
  if (!ctx || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(MI_ERR_BAD_ARG, "bad communicator arguments");
  return guarded([&]() -> int {
    ctx->use();
    if (ctx->comm) { MI_NCCL(Rccl::get().CommDestroy(ctx->comm)); ctx->comm = nullptr; }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof uid);
    MI_NCCL(Rccl::get().CommInitRank(&ctx->comm, n_ranks, uid, rank));
    ctx->rank = rank; ctx->n_ranks = n_ranks;
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();
    // Warm-up collective outside any stream capture: RCCL sets up its channels lazily on first use,
    // which must not happen while an iteration graph is being captured.
    ctx->scalar.ensure(1);
    MI_HIP(hipMemsetAsync(ctx->scalar.p, 0, sizeof(double), ctx->stream));
    ctx->allreduce(ctx->scalar.p, 1);
    MI_HIP(hipStreamSynchronize(ctx->stream));
    return MI_OK;
  });
}

// In-process "ranks" for single-GPU testing of the sharded paths (see LoopGroup in common.hpp).
int mi_loopback_group_create(int n_ranks, void **group) {
  if (!group || n_ranks < 1 || n_ranks > 64) return fail(MI_ERR_BAD_ARG, "bad loopback group arguments");
  return guarded([&]() -> int { *group = new LoopGroup(n_ranks); return MI_OK; });
}
int mi_loopback_group_destroy(void *group) {
  if (!group) return MI_OK;
  LoopGroup *g = static_cast<LoopGroup *>(group);
  for (auto e : g->ready) if (e) (void)hipEventDestroy(e);
  for (void *a : g->arena) if (a) (void)hipFree(a);
  delete g;
  return MI_OK;
}
static size_t peer_arena_default() {
  const int mb = env_int("MI355_PEER_ARENA_MB", 64);
  return (size_t)std::max(4, mb) << 20;
}
int mi_ctx_loopback_init(mi_ctx_t ctx, void *group, int rank) {
  LoopGroup *g = static_cast<LoopGroup *>(group);
  if (!ctx || !g || rank < 0 || rank >= g->n || ctx->comm) return fail(MI_ERR_BAD_ARG, "bad loopback arguments");
  return guarded([&]() -> int {
    ctx->use();
    ctx->loop = g; ctx->rank = rank; ctx->n_ranks = g->n;
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();
    // Device-side joining needs every rank's stream on a hardware queue of its own (a wait kernel at the head of a queue
    // it shares with the kernel it waits for never ends; measured: 8 streams on the default 4 queues expire every wait,
    // GPU_MAX_HW_QUEUES=16 runs them). Same answer on every rank: the environment is the process's.
    const bool device_side = g->mode == 0 && g->n <= XCHG_MAX_RANKS && env_int("GPU_MAX_HW_QUEUES", 4) >= g->n &&
                             !env_int("MI355_LOOPBACK_HOST", 0);
    if (!device_side) {
      ctx->no_graph = true;  // the host-rendezvous collective synchronises with the host
      return MI_OK;
    }
    delete ctx->peer;
    ctx->peer = new PeerComm();
    ctx->peer->init(ctx->device, rank, g->n, peer_arena_default());
    ctx->peer->owns_arena = false;                  // freed with the group: a rank that leaves early must not pull memory from under its peers' stores
    g->arena[rank] = ctx->peer->arena;
    g->barrier();                                   // every rank has published its arena
    for (int q = 0; q < g->n; ++q) ctx->peer->import_peer(q, nullptr, g->arena[q]);
    ctx->peer->finish();
    ctx->peer_on = true;
    ctx->no_graph = false;
    // Trial exchanges with a short bound: the ranks lined up by the host, then STAGGERED, each exchange between an
    // asynchronous copy in and one out — if two ranks' streams share a hardware queue (more live streams in the process
    // than GPU_MAX_HW_QUEUES), or the runtime puts the ranks' copies on one engine queue (a copy that waits for a
    // spinning kernel then blocks the next rank's copy in: measured with copies above GPU_FORCE_BLIT_COPY_SIZE), a wait
    // expires here instead of in a solve, and the whole group falls back to the host rendezvous.
    const long long keep = ctx->peer->peers.timeout;
    ctx->peer->set_timeout_ms(env_int("MI355_PEER_SELFTEST_MS", 400));
    const size_t trial = 16384;   // doubles: 128 KiB, above the runtime's default blit threshold
    ctx->pin_b.ensure(trial);
    DevBuf<double> tbuf(trial);
    ctx->peer->reserve_stage(trial);
    std::memset(ctx->pin_b.p, 0, trial * sizeof(double));
    for (int k = 0; k < 3; ++k) {
      g->barrier();
      std::this_thread::sleep_for(std::chrono::milliseconds(3 * ((rank + k) % g->n)));
      MI_HIP(hipMemcpyAsync(tbuf.p, ctx->pin_b.p, trial * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      ctx->peer->allreduce(tbuf.p, tbuf.p, trial, ctx->stream);
      MI_HIP(hipMemcpyAsync(ctx->pin_b.p, tbuf.p, trial * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      MI_HIP(hipStreamSynchronize(ctx->stream));
    }
    const int bad = ctx->peer->take_error(ctx->stream);
    { std::lock_guard<std::mutex> lk(g->mu); g->selftest_failed += bad; }
    g->barrier();
    ctx->peer->set_timeout_ticks(keep);
    if (g->selftest_failed) {
      ctx->peer_on = false;
      ctx->no_graph = true;
    }
    g->barrier();
    return MI_OK;
  });
}
int mi_loopback_group_set_mode(void *group, int mode) {
  if (!group || mode < 0 || mode > 1) return fail(MI_ERR_BAD_ARG, "bad loopback mode");
  static_cast<LoopGroup *>(group)->mode = mode;
  return MI_OK;
}

// ---- the peer exchange (exchange.hpp)
int mi_ctx_peer_init(mi_ctx_t ctx, int rank, int n_ranks, int64_t arena_bytes) {
  if (!ctx || arena_bytes < 0) return fail(MI_ERR_BAD_ARG, "bad peer-exchange arguments");
  return guarded([&]() -> int {
    ctx->use();
    MI_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();
    delete ctx->peer;
    ctx->peer = nullptr; ctx->peer_on = false;
    ctx->peer = new PeerComm();
    ctx->peer->init(ctx->device, rank, n_ranks, arena_bytes ? (size_t)arena_bytes : peer_arena_default());
    if (!ctx->comm) { ctx->rank = rank; ctx->n_ranks = n_ranks; }
    else if (ctx->rank != rank || ctx->n_ranks != n_ranks) raise(MI_ERR_BAD_ARG, "peer exchange: rank %d of %d differs from the communicator's %d of %d", rank, n_ranks, ctx->rank, ctx->n_ranks);
    return MI_OK;
  });
}
int mi_ctx_peer_export(mi_ctx_t ctx, void *handle_out, void **base_out) {
  if (!ctx || !ctx->peer || (!handle_out && !base_out)) return fail(MI_ERR_BAD_ARG, "peer exchange not initialised, or nothing to export into");
  return guarded([&]() -> int {
    ctx->use();
    if (handle_out) ctx->peer->export_handle(handle_out);
    if (base_out) *base_out = ctx->peer->arena;
    return MI_OK;
  });
}
int mi_ctx_peer_import(mi_ctx_t ctx, int rank, const void *handle, void *same_process_base) {
  if (!ctx || !ctx->peer) return fail(MI_ERR_BAD_ARG, "peer exchange not initialised");
  return guarded([&]() -> int { ctx->use(); ctx->peer->import_peer(rank, handle, same_process_base); return MI_OK; });
}
int mi_ctx_peer_ready(mi_ctx_t ctx) {
  if (!ctx || !ctx->peer) return fail(MI_ERR_BAD_ARG, "peer exchange not initialised");
  return guarded([&]() -> int { ctx->use(); ctx->peer->finish(); ctx->peer_on = true; return MI_OK; });
}
int mi_ctx_query(mi_ctx_t ctx, int what, int64_t *out) {
  if (!ctx || !out) return fail(MI_ERR_BAD_ARG, "bad query arguments");
  return guarded([&]() -> int {
    ctx->use();
    switch (what) {
      case MI_QUERY_NO_GRAPH: *out = ctx->no_graph ? 1 : 0; break;
      case MI_QUERY_PEER_EXCHANGE: *out = ctx->use_peer() ? (ctx->peer_inwait ? 3 : ctx->peer->fine_grained ? 2 : 1) : 0; break;
      case MI_QUERY_GRAPH_REPLAYS: *out = ctx->n_replays; break;
      case MI_QUERY_GRAPH_CAPTURES: *out = ctx->n_captures; break;
      case MI_QUERY_SPECTRAL_PINV: *out = spectral_pinv_calls().load(); break;
      case MI_QUERY_FOLDED_PCG: *out = folded_pcg_launches().load(); break;
      case MI_QUERY_EXPERIMENTAL: *out = 0; break;   // the EXPERIMENTAL build was removed
      case MI_QUERY_EXCHANGES: {
        unsigned long long e = 0;
        if (ctx->peer) {
          MI_HIP(hipStreamSynchronize(ctx->stream));
          memcpy_sync(&e, &ctx->peer->st->epoch, sizeof e, hipMemcpyDeviceToHost);
        }
        *out = (int64_t)e;
        break;
      }
      default: return fail(MI_ERR_BAD_ARG, "unknown query %d", what);
    }
    return MI_OK;
  });
}
int mi_ctx_set_exchange(mi_ctx_t ctx, int use_peer_exchange) {
  if (!ctx) return fail(MI_ERR_BAD_ARG, "ctx is NULL");
  if (use_peer_exchange && (!ctx->peer || !ctx->peer->ready)) return fail(MI_ERR_BAD_ARG, "peer exchange not ready");
  return guarded([&]() -> int {
    ctx->use();
    MI_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();
    ctx->peer_on = use_peer_exchange != 0;
    // (in-launch waits read the tables with no cache maintenance of their own: only with a fine-grained arena)
    ctx->peer_inwait = use_peer_exchange == 2 && ctx->peer && ctx->peer->fine_grained;
    return MI_OK;
  });
}

int mi_ctx_comm_destroy(mi_ctx_t ctx) {
  if (!ctx) return fail(MI_ERR_BAD_ARG, "ctx is NULL");
  return guarded([&]() -> int {
    ctx->use();
    MI_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &kv : ctx->workspaces) kv.second->drop_graphs();
    if (ctx->comm) MI_NCCL(Rccl::get().CommDestroy(ctx->comm));
    ctx->comm = nullptr; ctx->rank = 0; ctx->n_ranks = 1;
    return MI_OK;
  });
}

int mi_ctx_allreduce_sum(mi_ctx_t ctx, double *buf, int64_t n) {
  if (!ctx || !buf || n < 0) return fail(MI_ERR_BAD_ARG, "bad allreduce arguments");
  return guarded([&]() -> int {
    ctx->use();
    InOut v(ctx, buf, (size_t)n, ctx->scratch_a, true);
    ctx->allreduce(v.dev, (size_t)n);  // RCCL, the peer exchange or the in-process group's host rendezvous; a no-op without a communicator
    v.finish();
    if (ctx->use_peer() && !ctx->comm && ctx->peer->take_error(ctx->stream))
      raise(MI_ERR_COMM, "peer exchange: a wait for the other ranks expired (MI355_PEER_TIMEOUT_MS): %s", ctx->peer->err_text.c_str());
    return MI_OK;
  });
}

// ---------------------------------------------------------------- operators
#define MI_NEW_OP(ctx, op, expr)                                   \
  if (!(ctx) || !(op)) return fail(MI_ERR_BAD_ARG, "ctx/op is NULL"); \
  *(op) = nullptr;                                                 \
  return guarded([&]() -> int {                                    \
    (ctx)->use();                                                  \
    std::unique_ptr<mi_op_s> h(new mi_op_s);                       \
    h->impl.reset(expr);                                           \
    MI_HIP(hipStreamSynchronize((ctx)->stream));                   \
    *(op) = h.release();                                           \
    return MI_OK;                                                  \
  })

int mi_csr_create(mi_ctx_t ctx, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int64_t *colidx,
                  const double *val, int index_base, mi_op_t *op) {
  MI_NEW_OP(ctx, op, new CsrOp(ctx, host_csr(n_rows, n_cols, rowptr, colidx, val, index_base)));
}

int mi_diag_create(mi_ctx_t ctx, int64_t n, const double *dinv, mi_op_t *op) {
  if (n < 0 || n >= INT32_MAX) return fail(MI_ERR_BAD_ARG, "bad n");
  MI_NEW_OP(ctx, op, new DiagOp(ctx, n, dinv));
}

static SpdDirectOp *as_spd_direct(mi_op_t op) {
  return op && op->impl ? dynamic_cast<SpdDirectOp *>(op->impl.get()) : nullptr;
}
int mi_spd_direct_create(mi_ctx_t ctx, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval,
                         int index_base, mi_op_t *op) {
  if (!nzval) return fail(MI_ERR_BAD_ARG, "mi_spd_direct_create: nzval is NULL");
  MI_NEW_OP(ctx, op, new SpdDirectOp(ctx, n, colptr, rowval, nzval, index_base));
}
int mi_spd_direct_set_values(mi_op_t op, const double *nzval) {
  SpdDirectOp *d = as_spd_direct(op);
  if (!d || !nzval) return fail(MI_ERR_BAD_ARG, "mi_spd_direct_set_values: not a sparse direct preconditioner, or NULL nzval");
  mi_ctx_s *c = d->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> st;
    In vi(c, nzval, (size_t)d->nnz(), st);
    d->factor(vi.dev);   // synchronous: a singular matrix is reported here
    return MI_OK;
  });
}
int mi_spd_direct_stats(mi_op_t op, int64_t *pieces, int64_t *separator) {
  SpdDirectOp *d = as_spd_direct(op);
  if (!d) return fail(MI_ERR_BAD_ARG, "mi_spd_direct_stats: not a sparse direct preconditioner");
  if (pieces) *pieces = d->pl.n_pieces();
  if (separator) *separator = d->pl.n_sigma();
  return MI_OK;
}


static BlockJacobiOp *as_block_jacobi(mi_op_t op) { return op && op->impl ? dynamic_cast<BlockJacobiOp *>(op->impl.get()) : nullptr; }
int mi_block_jacobi_create(mi_ctx_t ctx, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, int64_t nb,
                           const int64_t *seed_ptr, const int64_t *seed_idx, int index_base, mi_op_t *op) {
  if (!nzval) return fail(MI_ERR_BAD_ARG, "mi_block_jacobi_create: nzval is NULL");
  MI_NEW_OP(ctx, op, new BlockJacobiOp(ctx, n, colptr, rowval, nzval, nb, seed_ptr, seed_idx, index_base));
}
int mi_block_jacobi_set_values(mi_op_t op, const double *nzval) {
  BlockJacobiOp *m = as_block_jacobi(op);
  if (!m || !nzval) return fail(MI_ERR_BAD_ARG, "mi_block_jacobi_set_values: not a block-Jacobi preconditioner, or NULL nzval");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    In vi(c, nzval, (size_t)m->nnz, m->stage);
    m->factor(vi.dev);   // synchronous: a singular or indefinite block is reported here
    return MI_OK;
  });
}
int mi_block_jacobi_stats(mi_op_t op, int64_t *n_g, int64_t *n_levels, int64_t *max_level, int64_t *kept_bytes) {
  BlockJacobiOp *m = as_block_jacobi(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_block_jacobi_stats: not a block-Jacobi preconditioner");
  for (int d = 0; d < m->nb; ++d) {
    if (n_g) n_g[d] = m->plan->dom[d].n_g;
    if (n_levels) n_levels[d] = m->plan->dom[d].nlev;
    if (max_level) max_level[d] = m->plan->dom[d].max_lev;
  }
  if (kept_bytes) *kept_bytes = m->kept;
  return MI_OK;
}

static AmgOp *as_amg(mi_op_t op) { return op && op->impl ? dynamic_cast<AmgOp *>(op->impl.get()) : nullptr; }
int mi_amg_create(mi_ctx_t ctx, int64_t nlevels, const int64_t *n_l, const int64_t *const *a_rowptr, const int64_t *const *a_colidx,
                  const double *const *a_val, const int64_t *const *p_rowptr, const int64_t *const *p_colidx, const double *const *p_val,
                  const double *omega_over_d, const double *coarse_inv, int index_base, mi_op_t *op) {
  if (op) *op = nullptr;
  if (nlevels < 1 || nlevels > 64) return fail(MI_ERR_BAD_ARG, "mi_amg_create: nlevels = %lld (1 <= nlevels <= 64)", (long long)nlevels);
  if (!n_l) return fail(MI_ERR_BAD_ARG, "mi_amg_create: n_l is NULL");
  MI_NEW_OP(ctx, op, new AmgOp(ctx, nlevels, n_l, a_rowptr, a_colidx, a_val, p_rowptr, p_colidx, p_val, omega_over_d, coarse_inv, index_base));
}
int mi_amg_stats(mi_op_t op, int64_t *n_levels, int64_t *coarse_n, int64_t *operator_nnz, int64_t *bytes_kept) {
  AmgOp *m = as_amg(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_amg_stats: not an AMG preconditioner");
  if (n_levels) *n_levels = m->nlev;
  if (coarse_n) *coarse_n = m->nc;
  if (operator_nnz) *operator_nnz = m->op_nnz;
  if (bytes_kept) *bytes_kept = m->kept;
  return MI_OK;
}
int mi_amg_plan_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, const double *val, int64_t nlevels,
                       const int64_t *n_l, const int64_t *const *agg, int index_base, mi_op_t *op) {
  if (op) *op = nullptr;
  if (!val) return fail(MI_ERR_BAD_ARG, "mi_amg_plan_create: val is NULL");
  MI_NEW_OP(ctx, op, new AmgPlanOp(ctx, n, rowptr, colidx, val, nlevels, n_l, agg, index_base));
}
int mi_amg_set_values(mi_op_t op, const double *val) {
  AmgPlanOp *m = op && op->impl ? dynamic_cast<AmgPlanOp *>(op->impl.get()) : nullptr;
  if (!m) return fail(MI_ERR_BAD_ARG, "%s", as_amg(op) ?"mi_amg_set_values: the hierarchy of this operator came from the host (mi_amg_create); only an "
                                                   "operator of mi_amg_plan_create can redo it"
                                                 : "mi_amg_set_values: not an AMG preconditioner");
  if (!val) return fail(MI_ERR_BAD_ARG, "mi_amg_set_values: val is NULL");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    In vi(c, val, (size_t)m->nnz0, m->stage);
    m->refresh(vi.dev, "mi_amg_set_values");   // synchronous: a matrix that is not positive definite is reported here
    return MI_OK;
  });
}
int mi_amg_refresh_profile(mi_op_t op, double *ms) {
  AmgPlanOp *m = op && op->impl ? dynamic_cast<AmgPlanOp *>(op->impl.get()) : nullptr;
  if (!m || !ms) return fail(MI_ERR_BAD_ARG, "mi_amg_refresh_profile: not an operator of mi_amg_plan_create, or NULL ms");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    m->profile(ms);
    return MI_OK;
  });
}
int mi_amg_level_sizes(mi_op_t op, int64_t level, int64_t *n_rows, int64_t *n_cols, int64_t *a_nnz, int64_t *p_nnz) {
  AmgOp *m = as_amg(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_amg_level_sizes: not an AMG preconditioner");
  if (level < 0 || level >= m->nlev) return fail(MI_ERR_BAD_ARG, "mi_amg_level_sizes: level = %lld of %d levels", (long long)level, m->nlev);
  m->level_sizes((int)level, n_rows, n_cols, a_nnz, p_nnz);
  return MI_OK;
}
int mi_amg_level_get(mi_op_t op, int64_t level, int64_t *a_rowptr, int64_t *a_colidx, double *a_val, int64_t *p_rowptr, int64_t *p_colidx,
                     double *p_val, double *omega, double *omega_over_d) {
  AmgOp *m = as_amg(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_amg_level_get: not an AMG preconditioner");
  if (level < 0 || level >= m->nlev) return fail(MI_ERR_BAD_ARG, "mi_amg_level_get: level = %lld of %d levels", (long long)level, m->nlev);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    m->level_get((int)level, a_rowptr, a_colidx, a_val, p_rowptr, p_colidx, p_val, omega, omega_over_d);
    return MI_OK;
  });
}
int mi_amg_coarse_inverse(mi_op_t op, double *coarse_inv) {
  AmgOp *m = as_amg(op);
  if (!m || !coarse_inv) return fail(MI_ERR_BAD_ARG, "mi_amg_coarse_inverse: not an AMG preconditioner, or NULL coarse_inv");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    MI_HIP(hipMemcpyAsync(coarse_inv, m->zinv.p, sizeof(double) * (size_t)m->nc * m->nc, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}

// new values of the stacked A_IΓ blocks of either operator on the interior/Γ split (host or device pointer)
static int split_set_values(SplitOp *m, const double *ig_val) {
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> st;
    In vi(c, ig_val, (size_t)m->nnz, st);
    m->set_values(vi.dev);
    MI_HIP(hipStreamSynchronize(c->stream));   // the staging buffer goes out of scope
    return MI_OK;
  });
}
static LorascOp *as_lorasc(mi_op_t op) { return op && op->impl ? dynamic_cast<LorascOp *>(op->impl.get()) : nullptr; }
int mi_lorasc_create(mi_ctx_t ctx, int64_t ndom, int64_t n, int64_t n_gamma, const int64_t *n_i, const int64_t *const *pos_I,
                     const int64_t *pos_gamma, const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                     const double *const *ig_nzval, mi_setup_t interior, mi_op_t a_gg_solver, int64_t nev, const double *E,
                     const double *coef, int index_base, mi_op_t *op) {
  if (op) *op = nullptr;
  if (dynamic_cast<AmgBankOp *>(a_gg_solver && a_gg_solver->impl ? a_gg_solver->impl.get() : nullptr))
    return fail(MI_ERR_BAD_ARG, "mi_lorasc_create: a_gg_solver is an AMG bank, which is not applicable itself; pass a view of it (mi_amg_bank_view)");
  MI_NEW_OP(ctx, op, new LorascOp(ctx, ndom, n, n_gamma, n_i, pos_I, pos_gamma, ig_colptr, ig_rowval, ig_nzval, interior, a_gg_solver,
                                  nev, E, coef, index_base));
}
int mi_lorasc_set_values(mi_op_t op, const double *ig_val) {
  LorascOp *l = as_lorasc(op);
  if (!l || !ig_val) return fail(MI_ERR_BAD_ARG, "mi_lorasc_set_values: not a LORASC preconditioner, or NULL ig_val");
  return split_set_values(l, ig_val);
}
int mi_lorasc_set_correction(mi_op_t op, int64_t nev, const double *E, const double *coef) {
  LorascOp *l = as_lorasc(op);
  if (!l) return fail(MI_ERR_BAD_ARG, "mi_lorasc_set_correction: not a LORASC preconditioner");
  mi_ctx_s *c = l->ctx;
  return guarded([&]() -> int {
    c->use();
    LorascOp::check_nev(nev, E, "mi_lorasc_set_correction");
    MI_HIP(hipStreamSynchronize(c->stream));
    for (auto &kv : c->workspaces) kv.second->drop_graphs_of(l);   // nev and the address of E are launch arguments of captured applies
    if (c->ptr_mode == MI_PTR_DEVICE) l->set_correction_dev(nev, E, coef);
    else l->set_correction_host(nev, E, coef, "mi_lorasc_set_correction");
    return MI_OK;
  });
}

static NnInducedOp *as_nn_induced(mi_op_t op) { return op && op->impl ? dynamic_cast<NnInducedOp *>(op->impl.get()) : nullptr; }
int mi_nn_induced_create(mi_ctx_t ctx, int64_t ndom, int64_t n, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *n_i,
                         const int64_t *const *pos_I, const int64_t *pos_gamma, const int64_t *const *gather_idx,
                         const int64_t *cnt, const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                         const double *const *ig_nzval, const double *const *PiSd, int storage, mi_setup_t interior,
                         int coupling, int index_base, mi_op_t *op) {
  MI_NEW_OP(ctx, op, new NnInducedOp(ctx, ndom, n, n_gamma, n_gamma_d, n_i, pos_I, pos_gamma, gather_idx, cnt, ig_colptr, ig_rowval,
                                     ig_nzval, PiSd, storage, interior, coupling, index_base));
}
int mi_nn_induced_set_values(mi_op_t op, const double *ig_val) {
  NnInducedOp *m = as_nn_induced(op);
  if (!m || !ig_val) return fail(MI_ERR_BAD_ARG, "mi_nn_induced_set_values: not a Neumann-Neumann induced preconditioner, or NULL ig_val");
  return split_set_values(m, ig_val);
}
int mi_nn_induced_set_coupling(mi_op_t op, int coupling) {
  NnInducedOp *m = as_nn_induced(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_nn_induced_set_coupling: not a Neumann-Neumann induced preconditioner");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    NnInducedOp::check_coupling(coupling, "mi_nn_induced_set_coupling");
    MI_HIP(hipStreamSynchronize(c->stream));
    for (auto &kv : c->workspaces) kv.second->drop_graphs_of(m);   // the index and operand arrays of launch 6 are arguments of captured applies
    m->coupling = coupling;
    return MI_OK;
  });
}

int mi_schur_assembled_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                              const int64_t *const *gather_idx, const double *const *Sd, int index_base,
                              int64_t dom_begin, int64_t dom_end, mi_op_t *op) {
  MI_NEW_OP(ctx, op, new DenseBlockOp(ctx, ndom, n_gamma, n_gamma_d, gather_idx, Sd, nullptr, index_base, dom_begin, dom_end));
}

int mi_nn_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *const *gather_idx,
                 const double *const *PiSd, const int64_t *node_gamma_cnt, int index_base, int64_t dom_begin,
                 int64_t dom_end, mi_op_t *op) {
  return mi_nn_create_stored(ctx, ndom, n_gamma, n_gamma_d, gather_idx, PiSd, node_gamma_cnt, index_base, dom_begin, dom_end,
                             MI_STORE_F64, op);
}
int mi_nn_create_stored(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *const *gather_idx,
                        const double *const *PiSd, const int64_t *node_gamma_cnt, int index_base, int64_t dom_begin,
                        int64_t dom_end, int storage, mi_op_t *op) {
  if (op) *op = nullptr;
  if (storage != MI_STORE_F64 && storage != MI_STORE_F32) return fail(MI_ERR_BAD_ARG, "mi_nn_create_stored: unknown storage %d", storage);
  if (!node_gamma_cnt) return fail(MI_ERR_BAD_ARG, "node_gamma_cnt is NULL");
  MI_NEW_OP(ctx, op, new DenseBlockOp(ctx, ndom, n_gamma, n_gamma_d, gather_idx, PiSd, node_gamma_cnt, index_base, dom_begin, dom_end, storage));
}
int mi_op_storage(mi_op_t op, int *storage) {
  if (!op || !op->impl || !storage) return fail(MI_ERR_BAD_ARG, "mi_op_storage: NULL argument");
  DenseBlockOp *d = op->impl->as_dense();
  *storage = d ? d->storage : MI_STORE_F64;
  return MI_OK;
}

int mi_schur_matfree_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d, const int64_t *n_i,
                            const int64_t *const *gather_idx, const int64_t *const *ig_colptr,
                            const int64_t *const *ig_rowval, const double *const *ig_nzval,
                            const int64_t *const *gg_colptr, const int64_t *const *gg_rowval,
                            const double *const *gg_nzval, mi_interior_solve_fn solve, void *user, int index_base,
                            int64_t dom_begin, int64_t dom_end, mi_op_t *op) {
  MI_NEW_OP(ctx, op, new MatfreeSchurOp(ctx, ndom, n_gamma, n_gamma_d, n_i, gather_idx, ig_colptr, ig_rowval, ig_nzval,
                                        gg_colptr, gg_rowval, gg_nzval, solve, user, index_base, dom_begin, dom_end));
}

int mi_schur_matfree_device_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_gamma_d,
                                   const int64_t *n_i, const int64_t *const *gather_idx,
                                   const int64_t *const *ii_colptr, const int64_t *const *ii_rowval,
                                   const double *const *ii_nzval, const int64_t *const *ig_colptr,
                                   const int64_t *const *ig_rowval, const double *const *ig_nzval,
                                   const int64_t *const *gg_colptr, const int64_t *const *gg_rowval,
                                   const double *const *gg_nzval, double reltol, int index_base, int64_t dom_begin,
                                   int64_t dom_end, mi_op_t *op) {
  if (!ii_colptr) return fail(MI_ERR_BAD_ARG, "A_II arrays are NULL");
  MI_NEW_OP(ctx, op, new MatfreeSchurOp(ctx, ndom, n_gamma, n_gamma_d, n_i, gather_idx, ig_colptr, ig_rowval, ig_nzval,
                                        gg_colptr, gg_rowval, gg_nzval, nullptr, nullptr, index_base, dom_begin, dom_end,
                                        ii_colptr, ii_rowval, ii_nzval, reltol));
}

int mi_schur_global_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_i,
                           const int64_t *const *ig_colptr, const int64_t *const *ig_rowval,
                           const double *const *ig_nzval, const int64_t *gg_colptr, const int64_t *gg_rowval,
                           const double *gg_nzval, mi_interior_solve_fn solve, void *user, int index_base, mi_op_t *op) {
  MI_NEW_OP(ctx, op, new GlobalSchurOp(ctx, ndom, n_gamma, n_i, ig_colptr, ig_rowval, ig_nzval, gg_colptr, gg_rowval,
                                       gg_nzval, solve, user, index_base));
}

int mi_schur_global_device_create(mi_ctx_t ctx, int64_t ndom, int64_t n_gamma, const int64_t *n_i,
                                  const int64_t *const *ii_colptr, const int64_t *const *ii_rowval,
                                  const double *const *ii_nzval, const int64_t *const *ig_colptr,
                                  const int64_t *const *ig_rowval, const double *const *ig_nzval,
                                  const int64_t *gg_colptr, const int64_t *gg_rowval, const double *gg_nzval,
                                  double reltol, int index_base, mi_op_t *op) {
  if (!ii_colptr) return fail(MI_ERR_BAD_ARG, "mi_schur_global_device_create: A_II arrays are NULL");
  MI_NEW_OP(ctx, op, new GlobalSchurOp(ctx, ndom, n_gamma, n_i, ig_colptr, ig_rowval, ig_nzval, gg_colptr, gg_rowval,
                                       gg_nzval, nullptr, nullptr, index_base, ii_colptr, ii_rowval, ii_nzval, reltol));
}

static AmgBankOp *as_amg_bank(mi_op_t op);
int mi_op_size(mi_op_t op, int64_t *n) {
  if (!op || !op->impl || !n) return fail(MI_ERR_BAD_ARG, "NULL argument");
  *n = op->impl->n;
  return MI_OK;
}

int mi_op_apply(mi_op_t op, const double *x, double *y) {
  if (!op || !op->impl || !x || !y || x == y) return fail(MI_ERR_BAD_ARG, "mi_op_apply: NULL or aliased argument");
  if (int rc = refuse_unusable("mi_op_apply", {op})) return rc;
  return guarded([&]() -> int {
    mi_ctx_s *c = op->impl->ctx;
    c->use();
    const size_t n = (size_t)op->impl->n;
    if (n == 0) return MI_OK;   // an empty operator: nothing to copy or launch (its staging buffers were never allocated)
    if (c->ptr_mode == MI_PTR_DEVICE) {
      op->impl->apply(x, y, nullptr);
      return MI_OK;
    }
    // Host pointers (the reference's own Julia loop calling mul! / \ every iteration): through pinned buffers, so both
    // copies are plain DMA transfers instead of the runtime's staged pageable copies.
    static const bool trace = env_int("MI355_TRACE", 0) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto tr = [&](const char *what) {
      if (trace) std::fprintf(stderr, "[trace rank %d] mi_op_apply %-22s +%.3f s\n", c->rank, what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    };
    c->pin_b.ensure(n); c->pin_x.ensure(n);
    tr("pinned buffers");
    op->hx.ensure(n); op->hy.ensure(n);
    tr("device buffers");
    std::memcpy(c->pin_b.p, x, n * sizeof(double));
    MI_HIP(hipMemcpyAsync(op->hx.p, c->pin_b.p, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    tr("H2D enqueued");
    if (c->has_comm() || !op->impl->writes_y_once()) {  // a collective or read-modify-write kernels touch y: keep it in device memory
      op->impl->apply(op->hx.p, op->hy.p, nullptr);
      tr("apply enqueued");
      MI_HIP(hipMemcpyAsync(c->pin_x.p, op->hy.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      tr("D2H enqueued");
    } else {
      op->impl->apply(op->hx.p, c->pin_x.p, nullptr);  // the last kernel of the apply writes y straight into pinned memory
    }
    MI_HIP(hipStreamSynchronize(c->stream));
    tr("synchronised");
    std::memcpy(y, c->pin_x.p, n * sizeof(double));
    return MI_OK;
  });
}

int mi_op_bytes(mi_op_t op, int64_t *bytes_apply, int64_t *bytes_dominant_kernel) {
  if (!op || !op->impl) return fail(MI_ERR_BAD_ARG, "op is NULL");
  int64_t a = 0, d = 0;
  op->impl->bytes(&a, &d);
  if (bytes_apply) *bytes_apply = a;
  if (bytes_dominant_kernel) *bytes_dominant_kernel = d;
  return MI_OK;
}

// Launch the dominant kernel `reps` times. With `us_per_launch` the launches are replayed from one graph
// (eager launches of a ~5 us kernel are bound by the host's launch rate) between two HIP events recorded on the
// context's stream, after a warm-up replay; the average duration per launch is returned.
static int dominant_impl(mi_op_t op, const double *x, int reps, double *us_per_launch) {
  if (!op || !op->impl || !x || reps < 0) return fail(MI_ERR_BAD_ARG, "bad argument");
  if (int rc = refuse_unusable(us_per_launch ? "mi_op_time_dominant" : "mi_op_apply_dominant", {op})) return rc;
  return guarded([&]() -> int {
    mi_ctx_s *c = op->impl->ctx;
    c->use();
    In xi(c, x, (size_t)op->impl->n, op->hx);
    if (!us_per_launch) {
      for (int i = 0; i < reps; ++i) op->impl->apply_dominant(xi.dev);
      return MI_OK;
    }
    *us_per_launch = 0.0;
    if (reps == 0) return MI_OK;
    hipStream_t s = c->stream;
    hipGraphExec_t ex = capture_graph(s, "", [&] { for (int i = 0; i < reps; ++i) op->impl->apply_dominant(xi.dev); });
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipGraphLaunch(ex, s);           // warm-up replay
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    if (e == hipSuccess) e = hipGraphLaunch(ex, s);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipGraphExecDestroy(ex);
    if (e != hipSuccess) raise(MI_ERR_HIP, "timed replay failed: %s", hipGetErrorString(e));
    *us_per_launch = (double)ms * 1e3 / reps;
    return MI_OK;
  });
}

int mi_op_apply_dominant(mi_op_t op, const double *x, int reps) { return dominant_impl(op, x, reps, nullptr); }

int mi_op_time_dominant(mi_op_t op, const double *x, int reps, double *us_per_launch) {
  if (!us_per_launch) return fail(MI_ERR_BAD_ARG, "us_per_launch is NULL");
  return dominant_impl(op, x, reps, us_per_launch);
}

int mi_op_destroy(mi_op_t op) {
  if (!op) return MI_OK;
  if (op->bound > 0) return fail(MI_ERR_BAD_ARG, "mi_op_destroy: %d live LORASC operator(s) use this operator; destroy them first", op->bound);
  if (op->bound_combine > 0)
    return fail(MI_ERR_BAD_ARG, "mi_op_destroy: this operator holds %d place(s) among the children of live combined operator(s) (mi_op_combine); destroy them first", op->bound_combine);
  if (AmgBankOp *bk = as_amg_bank(op))
    if (bk->views > 0) return fail(MI_ERR_BAD_ARG, "mi_op_destroy: %d live view(s) (mi_amg_bank_view) borrow this AMG bank; destroy them first", bk->views);
  return guarded([&]() -> int {
    if (op->impl) {
      mi_ctx_s *c = op->impl->ctx;
      c->use();
      (void)hipStreamSynchronize(c->stream);
      for (auto &kv : c->workspaces) kv.second->drop_graphs_of(op->impl.get());
    }
    delete op;
    return MI_OK;
  });
}

// ---------------------------------------------------------------- BLAS-1
int mi_dot(mi_ctx_t ctx, int64_t n, const double *x, const double *y, double *result) {
  if (!ctx || n < 0 || n >= INT32_MAX || !x || !y || !result) return fail(MI_ERR_BAD_ARG, "mi_dot: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    In xi(ctx, x, (size_t)n, ctx->scratch_a), yi(ctx, y, (size_t)n, ctx->scratch_b);
    const int g = vec_grid(n);
    hipLaunchKernelGGL(k_dot_partial, dim3(g), dim3(NT), 0, ctx->stream, (int)n, xi.dev, yi.dev, ctx->partials.p,
                       (const int *)nullptr);
    *result = reduce_to_host(ctx, g, 0);
    return MI_OK;
  });
}

int mi_norm2(mi_ctx_t ctx, int64_t n, const double *x, double *result) {
  if (!ctx || n < 0 || n >= INT32_MAX || !x || !result) return fail(MI_ERR_BAD_ARG, "mi_norm2: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    In xi(ctx, x, (size_t)n, ctx->scratch_a);
    const int g = vec_grid(n);
    hipLaunchKernelGGL(k_dot_partial, dim3(g), dim3(NT), 0, ctx->stream, (int)n, xi.dev, xi.dev, ctx->partials.p,
                       (const int *)nullptr);
    *result = reduce_to_host(ctx, g, 1);
    return MI_OK;
  });
}

int mi_axpy(mi_ctx_t ctx, int64_t n, double a, const double *x, double *y) {
  if (!ctx || n < 0 || n >= INT32_MAX || !x || !y) return fail(MI_ERR_BAD_ARG, "mi_axpy: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    In xi(ctx, x, (size_t)n, ctx->scratch_a);
    InOut yo(ctx, y, (size_t)n, ctx->scratch_b, true);
    hipLaunchKernelGGL(k_axpy, dim3(vec_grid(n)), dim3(NT), 0, ctx->stream, (int)n, a, xi.dev, yo.dev);
    MI_HIP(hipGetLastError());
    yo.finish();
    return MI_OK;
  });
}

int mi_axpby(mi_ctx_t ctx, int64_t n, double a, const double *x, double b, double *y) {
  if (!ctx || n < 0 || n >= INT32_MAX || !x || !y) return fail(MI_ERR_BAD_ARG, "mi_axpby: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    In xi(ctx, x, (size_t)n, ctx->scratch_a);
    InOut yo(ctx, y, (size_t)n, ctx->scratch_b, true);
    hipLaunchKernelGGL(k_axpby, dim3(vec_grid(n)), dim3(NT), 0, ctx->stream, (int)n, a, xi.dev, b, yo.dev);
    MI_HIP(hipGetLastError());
    yo.finish();
    return MI_OK;
  });
}

// ---------------------------------------------------------------- solvers
int mi_cg(mi_op_t A, const double *b, double *x, int64_t maxit, double eps, double *res_norm, int64_t res_cap,
          int64_t *it) {
  return run_solver(A, nullptr, b, x, nullptr, 0, maxit, eps, res_norm, res_cap, it, false, false);
}
int mi_pcg(mi_op_t A, mi_op_t M, const double *b, double *x, int64_t maxit, double eps, double *res_norm,
           int64_t res_cap, int64_t *it) {
  return run_solver(A, M, b, x, nullptr, 0, maxit, eps, res_norm, res_cap, it, true, false);
}
int mi_defcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit, double eps,
             double *res_norm, int64_t res_cap, int64_t *it) {
  return run_solver(A, nullptr, b, x, W, nvec, maxit, eps, res_norm, res_cap, it, false, true);
}
int mi_defpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit,
              double eps, double *res_norm, int64_t res_cap, int64_t *it) {
  return run_solver(A, M, b, x, W, nvec, maxit, eps, res_norm, res_cap, it, true, true);
}

int mi_eigcg(mi_op_t A, const double *b, double *x, int64_t nvec, int64_t spdim, int64_t maxit, double eps,
             double *res_norm, int64_t res_cap, int64_t *it, double *V_out) {
  return run_eig_solver(EIGCG, A, nullptr, b, x, nullptr, nvec, spdim, maxit, eps, res_norm, res_cap, it, V_out);
}
int mi_eigpcg(mi_op_t A, mi_op_t M, const double *b, double *x, int64_t nvec, int64_t spdim, int64_t maxit, double eps,
              double *res_norm, int64_t res_cap, int64_t *it, double *V_out) {
  return run_eig_solver(EIGPCG, A, M, b, x, nullptr, nvec, spdim, maxit, eps, res_norm, res_cap, it, V_out);
}
int mi_eigdefcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t spdim, int64_t maxit,
                double eps, double *res_norm, int64_t res_cap, int64_t *it, double *V_out) {
  return run_eig_solver(EIGDEFCG, A, nullptr, b, x, W, nvec, spdim, maxit, eps, res_norm, res_cap, it, V_out);
}
int mi_eigdefpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t spdim,
                 int64_t maxit, double eps, double *res_norm, int64_t res_cap, int64_t *it, double *V_out) {
  return run_eig_solver(EIGDEFPCG, A, M, b, x, W, nvec, spdim, maxit, eps, res_norm, res_cap, it, V_out);
}
int mi_initcg(mi_op_t A, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit, double eps,
              double *res_norm, int64_t res_cap, int64_t *it) {
  return run_init_solver(A, nullptr, b, x, W, nvec, maxit, eps, res_norm, res_cap, it, false);
}
int mi_initpcg(mi_op_t A, mi_op_t M, const double *b, double *x, const double *W, int64_t nvec, int64_t maxit, double eps,
               double *res_norm, int64_t res_cap, int64_t *it) {
  return run_init_solver(A, M, b, x, W, nvec, maxit, eps, res_norm, res_cap, it, true);
}

// ---------------------------------------------------------------- eigensolver (lanczos.hpp)
int mi_eigsolve(mi_op_t A, mi_op_t B, mi_op_t Binv, int64_t nev, int which, int64_t krylovdim, double tol, int64_t maxiter,
                const double *v0, double *vals, double *vecs, double *resid, int64_t *nconv, int64_t *nrestart, int64_t *napply) {
  if (!A || !A->impl || !vals || !vecs) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: A, vals or vecs is NULL");
  if ((B == nullptr) != (Binv == nullptr))
    return fail(MI_ERR_BAD_ARG, "mi_eigsolve: B and Binv go together (both NULL: the standard problem)");
  if (B && (!B->impl || !Binv->impl)) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: B or Binv is an empty handle");
  Operator *a = A->impl.get(), *b = B ? B->impl.get() : nullptr, *bi = B ? Binv->impl.get() : nullptr;
  const int64_t n = a->n;
  if (b && (b->n != n || bi->n != n || b->ctx != a->ctx || bi->ctx != a->ctx))
    return fail(MI_ERR_BAD_ARG, "mi_eigsolve: A (%lld), B (%lld) and Binv (%lld) differ in size or context", (long long)n,
                (long long)b->n, (long long)bi->n);
  if (nev < 1 || nev > n) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: nev = %lld outside [1, n = %lld]", (long long)nev, (long long)n);
  if (which != MI_EIG_SR && which != MI_EIG_LR) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: which = %d is neither MI_EIG_SR nor MI_EIG_LR", which);
  if (krylovdim < 0 || (krylovdim != 0 && krylovdim < nev + 1 && krylovdim < n))
    return fail(MI_ERR_BAD_ARG, "mi_eigsolve: krylovdim = %lld; 0 or at least nev + 1 = %lld (or n = %lld) expected", (long long)krylovdim,
                (long long)(nev + 1), (long long)n);
  if (!(tol >= 0.0) || maxiter < 0) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: tol = %g, maxiter = %lld: both must be non-negative", tol, (long long)maxiter);
  const int64_t m = std::min<int64_t>(krylovdim ? krylovdim : std::max<int64_t>(2 * nev, 8), n);
  if (m > 1024) return fail(MI_ERR_BAD_ARG, "mi_eigsolve: a window of %lld columns; at most 1024 are supported", (long long)m);
  mi_ctx_s *c = a->ctx;
  if (c->has_comm())
    return fail(MI_ERR_BAD_ARG, "mi_eigsolve: the context is one rank of several; sharded eigensolves are not provided");
  if (int rc = refuse_unusable("mi_eigsolve", {A, B, Binv})) return rc;
  return guarded([&]() -> int {
    c->use();
    In vi(c, v0, v0 ? (size_t)n : 0, c->scratch_a);
    DevBuf<double> xstage;
    InOut xo(c, vecs, (size_t)n * (size_t)nev, xstage, false);
    LanczosResult r;
    int rc;
    {
      Lanczos lz(c, a, b, bi, (int)nev, which, (int)m);
      rc = lz.solve(v0 ? vi.dev : nullptr, tol, maxiter, xo.dev, r);
      MI_HIP(hipStreamSynchronize(c->stream));   // the panels go back to the pool behind this brace
    }
    if (rc != MI_OK) return rc;
    xo.finish();
    std::copy(r.vals.begin(), r.vals.end(), vals);
    if (resid) std::copy(r.resid.begin(), r.resid.end(), resid);
    if (nconv) *nconv = r.nconv;
    if (nrestart) *nrestart = r.nrestart;
    if (napply) *napply = r.napply;
    return MI_OK;
  });
}

// ---------------------------------------------------------------- Karhunen-Loève: covariance kernel and C = M K M (kl.hpp)
int mi_cov_tiling(int64_t nt, int64_t ns, int64_t m, int64_t *row_tile, int64_t *src_chunk, int64_t *col_block, int64_t *splits) {
  if (nt < 1 || ns < 1 || m < 1) return fail(MI_ERR_BAD_ARG, "mi_cov_tiling: nt = %lld, ns = %lld, m = %lld: all must be at least 1", (long long)nt, (long long)ns, (long long)m);
  if (row_tile) *row_tile = COV_ROW_TILE;
  if (src_chunk) *src_chunk = COV_SRC_CHUNK;
  if (col_block) *col_block = COV_CB;
  if (splits) *splits = cov_tiling(nt, ns, m).splits;
  return MI_OK;
}

int mi_cov_apply(mi_ctx_t ctx, int model, double sig2, double L, int64_t nt, const double *pt, int64_t ns, const double *ps,
                 int64_t m, const double *X, int64_t ldx, double *Y, int64_t ldy) {
  const char *me = "mi_cov_apply";
  if (!ctx || !pt || !ps || !X || !Y) return fail(MI_ERR_BAD_ARG, "%s: ctx, pt, ps, X or Y is NULL", me);
  const int64_t cap = (int64_t)1 << 30;
  if (nt < 1 || ns < 1 || m < 1 || nt > cap || ns > cap || m > 65535 * (int64_t)COV_CB)
    return fail(MI_ERR_BAD_ARG, "%s: nt = %lld, ns = %lld, m = %lld: each at least 1 (nt, ns at most 2^30)", me, (long long)nt, (long long)ns, (long long)m);
  if (ldx < ns || ldy < nt)
    return fail(MI_ERR_BAD_ARG, "%s: ldx = %lld < ns = %lld or ldy = %lld < nt = %lld", me, (long long)ldx, (long long)ns, (long long)ldy, (long long)nt);
  if (ctx->has_comm()) return fail(MI_ERR_BAD_ARG, "%s: the context is one rank of several; sharded covariance applies are not provided", me);
  return guarded([&]() -> int {
    cov_check_model(me, model, sig2, L);
    ctx->use();
    hipStream_t s = ctx->stream;
    DevBuf<double> work(std::max<size_t>(1, cov_workspace(nt, ns, m)));
    if (ctx->ptr_mode == MI_PTR_DEVICE) {
      cov_launch(s, model, sig2, L, (int)nt, pt, (int)ns, ps, (int)m, X, ldx, Y, ldy, work.p, nullptr);
      MI_HIP(hipGetLastError());
      MI_HIP(hipStreamSynchronize(s));   // the workspace goes back to the pool behind this brace
      return MI_OK;
    }
    cov_check_points(me, "pt", pt, nt);
    if (ps != pt) cov_check_points(me, "ps", ps, ns);
    DevBuf<double> dpt(2 * (size_t)nt), dps, dX((size_t)ns * m), dY((size_t)nt * m);
    MI_HIP(hipMemcpyAsync(dpt.p, pt, sizeof(double) * 2 * (size_t)nt, hipMemcpyHostToDevice, s));
    const double *src = dpt.p;
    if (ps != pt) {
      dps.alloc(2 * (size_t)ns);
      MI_HIP(hipMemcpyAsync(dps.p, ps, sizeof(double) * 2 * (size_t)ns, hipMemcpyHostToDevice, s));
      src = dps.p;
    }
    // rows [0, ns) of every column only: the padding up to ldx is not the caller's to be read
    MI_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)ns, X, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)ns, (size_t)m,
                            hipMemcpyHostToDevice, s));
    cov_launch(s, model, sig2, L, (int)nt, dpt.p, (int)ns, src, (int)m, dX.p, ns, dY.p, nt, work.p, nullptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpy2DAsync(Y, sizeof(double) * (size_t)ldy, dY.p, sizeof(double) * (size_t)nt, sizeof(double) * (size_t)nt, (size_t)m,
                            hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    return MI_OK;
  });
}

int mi_kl_cov_create(mi_ctx_t ctx, int model, double sig2, double L, int64_t n, const double *points, const int64_t *m_rowptr,
                     const int64_t *m_colidx, const double *m_val, mi_op_t *op) {
  const char *me = "mi_kl_cov_create";
  if (op) *op = nullptr;
  if (!ctx || !op || !points || !m_rowptr || !m_colidx || !m_val) return fail(MI_ERR_BAD_ARG, "%s: ctx, op, points or an array of M is NULL", me);
  if (n < 1 || n > ((int64_t)1 << 30)) return fail(MI_ERR_BAD_ARG, "%s: n = %lld (1 <= n <= 2^30)", me, (long long)n);
  if (ctx->has_comm()) return fail(MI_ERR_BAD_ARG, "%s: the context is one rank of several; sharded KL operators are not provided", me);
  MI_NEW_OP(ctx, op, ([&]() -> Operator * {
    cov_check_model(me, model, sig2, L);
    cov_check_points(me, "points", points, n);
    HostCsr hm;
    try {
      hm = host_csr(n, n, m_rowptr, m_colidx, m_val, 0);
    } catch (const Error &e) {
      const std::string why = last_error();
      raise(e.code, "%s: M is not a %lld x %lld CSR matrix: %s", me, (long long)n, (long long)n, why.c_str());
    }
    for (double v : hm.val)
      if (!std::isfinite(v)) raise(MI_ERR_BAD_ARG, "%s: M holds %g (not finite)", me, v);
    return new KlCovOp(ctx, model, sig2, L, n, points, hm);
  })());
}

// ---------------------------------------------------------------- realization sampler: ξ -> g -> a = exp(g) (kl_field.hpp)
int mi_kl_field_tiling(int64_t n, int64_t m, int64_t nreal, int64_t *row_tile, int64_t *mode_chunk, int64_t *real_block, int64_t *coord_splits) {
  if (n < 1 || m < 1 || nreal < 1 || n > KLF_MAX_N || m > KLF_MAX_N || nreal > KLF_MAX_N)
    return fail(MI_ERR_BAD_ARG, "mi_kl_field_tiling: n = %lld, m = %lld, nreal = %lld: each at least 1 and at most 2^30", (long long)n, (long long)m, (long long)nreal);
  if (row_tile) *row_tile = KLF_ROW_TILE;
  if (mode_chunk) *mode_chunk = KLF_MODE_CHUNK;
  if (real_block) *real_block = KLF_RB;
  if (coord_splits) *coord_splits = klf_tiling(n, m, nreal).coord_splits;
  return MI_OK;
}

// the checks both constructors share; NULL after a refusal (mi_last_error is set)
static mi_kl_field_s *klf_new(const char *me, mi_ctx_t ctx, int64_t n, int64_t m, const double *lam, int *rc) {
  *rc = MI_ERR_BAD_ARG;
  if (!ctx || !lam) { fail(MI_ERR_BAD_ARG, "%s: ctx or Lambda is NULL", me); return nullptr; }
  if (n < 1 || m < 1 || n > KLF_MAX_N || m > KLF_MAX_N) {
    fail(MI_ERR_BAD_ARG, "%s: n = %lld, m = %lld: each at least 1 and at most 2^30", me, (long long)n, (long long)m);
    return nullptr;
  }
  if (ctx->has_comm()) { fail(MI_ERR_BAD_ARG, "%s: the context is one rank of several; sharded KL fields are not provided", me); return nullptr; }
  for (int64_t a = 0; a < m; ++a)
    if (!(lam[a] >= 0.0) || !std::isfinite(lam[a])) {
      fail(MI_ERR_BAD_ARG, "%s: Lambda[%lld] = %g is negative or not finite (the reference's sqrt would throw)", me, (long long)a, lam[a]);
      return nullptr;
    }
  *rc = MI_OK;
  mi_kl_field_s *f = new mi_kl_field_s;
  f->ctx = ctx; f->n = (int)n; f->m = (int)m;
  f->lam.assign(lam, lam + m);
  return f;
}
static void klf_upload_common(mi_kl_field_s *f) {
  std::vector<double> sq(f->lam.size());
  for (size_t a = 0; a < sq.size(); ++a) sq[a] = std::sqrt(f->lam[a]);   // correctly rounded, as the host's sqrt(Λ[α])
  f->sqrt_lam.upload(sq, f->ctx->stream);
  f->c.alloc((size_t)f->m * KLF_RB);
}
// column-major host matrix (rows x cols, leading dimension ld) -> compact device matrix; blocking
static void klf_upload_matrix(mi_ctx_s *c, DevBuf<double> &dst, const double *src, size_t rows, size_t cols, size_t ld) {
  dst.alloc(rows * cols);
  MI_HIP(hipMemcpy2DAsync(dst.p, sizeof(double) * rows, src, sizeof(double) * ld, sizeof(double) * rows, cols, hipMemcpyHostToDevice, c->stream));
  MI_HIP(hipStreamSynchronize(c->stream));
}

int mi_kl_field_create(mi_ctx_t ctx, int64_t n, int64_t m, const double *lambda, const double *Psi, int64_t ldpsi, mi_kl_field_t *field) {
  const char *me = "mi_kl_field_create";
  if (!field) return fail(MI_ERR_BAD_ARG, "%s: field is NULL", me);
  *field = nullptr;
  if (!Psi) return fail(MI_ERR_BAD_ARG, "%s: Psi is NULL", me);
  if (ldpsi < n) return fail(MI_ERR_BAD_ARG, "%s: ldpsi = %lld < n = %lld", me, (long long)ldpsi, (long long)n);
  return guarded([&]() -> int {
    int rc;
    std::unique_ptr<mi_kl_field_s> f(klf_new(me, ctx, n, m, lambda, &rc));
    if (!f) return rc;
    ctx->use();
    klf_upload_common(f.get());
    klf_upload_matrix(ctx, f->Psi, Psi, (size_t)n, (size_t)m, (size_t)ldpsi);
    f->w.alloc((size_t)n);
    f->part.alloc((size_t)klf_tiling(n, m, 1).coord_splits * (size_t)m);
    f->bytes_kept = 8 * (n * m + m);
    f->bytes_per_set = 8 * (n * m + 4 * m + n);   // Ψ; sqrt(Λ) and ξ in, c out and in; one output
    *field = f.release();
    return MI_OK;
  });
}

int mi_kl_field_create_dd(mi_ctx_t ctx, int64_t n, int64_t m, const double *lambda, int64_t ndom, const int64_t *n_d, const int64_t *md,
                          const int64_t *inds_l2gd, int index_base, const double *Phid, const double *Phi, int64_t ldphi,
                          mi_kl_field_t *field) {
  const char *me = "mi_kl_field_create_dd";
  if (!field) return fail(MI_ERR_BAD_ARG, "%s: field is NULL", me);
  *field = nullptr;
  if (!n_d || !md || !inds_l2gd || !Phid || !Phi) return fail(MI_ERR_BAD_ARG, "%s: n_d, md, inds_l2gd, Phid or Phi is NULL", me);
  return guarded([&]() -> int {
    int rc;
    std::unique_ptr<mi_kl_field_s> f(klf_new(me, ctx, n, m, lambda, &rc));
    if (!f) return rc;
    std::string err;
    if (klfp::make_dd_plan(n, ndom, n_d, md, inds_l2gd, index_base, f->plan, err) != klfp::OK) return fail(MI_ERR_BAD_ARG, "%s: %s", me, err.c_str());
    const klfp::Plan &pl = f->plan;
    if (ldphi < pl.nred) return fail(MI_ERR_BAD_ARG, "%s: ldphi = %lld < the %lld rows of Phi (the sum of md)", me, (long long)ldphi, (long long)pl.nred);
    f->dd = true;
    ctx->use();
    hipStream_t s = ctx->stream;
    klf_upload_common(f.get());
    klf_upload_matrix(ctx, f->Phi, Phi, (size_t)pl.nred, (size_t)m, (size_t)ldphi);
    f->Phid.upload(Phid, (size_t)pl.phid_off.back(), s);
    MI_HIP(hipStreamSynchronize(s));
    f->tiles.upload(pl.tiles, s); f->n_d.upload(pl.n_d, s); f->md.upload(pl.md, s); f->y_off.upload(pl.y_off, s); f->t_off.upload(pl.t_off, s);
    f->phid_off.upload(pl.phid_off, s); f->own_ptr.upload(pl.own_ptr, s); f->own_pos.upload(pl.own_pos, s);
    f->y.alloc((size_t)pl.nred * KLF_RB);
    f->t.alloc((size_t)pl.nloc * KLF_RB);
    const int64_t factors = 8 * ((int64_t)pl.phid_off.back() + (int64_t)pl.nred * m);
    f->bytes_kept = factors + 8 * m + pl.bytes();
    // the factors, c, y written and read, t written and read, the owner lists, one output
    f->bytes_per_set = factors + 8 * 4 * m + 16 * (int64_t)pl.nred + 16 * (int64_t)pl.nloc + 4 * ((int64_t)n + 1 + pl.nloc) + 8 * n;
    *field = f.release();
    return MI_OK;
  });
}

int mi_kl_field_set(mi_kl_field_t field, int64_t nreal, const double *Xi, int64_t ldxi, double *G, int64_t ldg, double *A, int64_t lda) {
  const char *me = "mi_kl_field_set";
  if (!field || !Xi) return fail(MI_ERR_BAD_ARG, "%s: field or Xi is NULL", me);
  if (!G && !A) return fail(MI_ERR_BAD_ARG, "%s: G and A are both NULL", me);
  if (nreal < 1 || nreal > KLF_MAX_N) return fail(MI_ERR_BAD_ARG, "%s: nreal = %lld (1 <= nreal <= 2^30)", me, (long long)nreal);
  const int64_t n = field->n, m = field->m;
  if (ldxi < m || (G && ldg < n) || (A && lda < n))
    return fail(MI_ERR_BAD_ARG, "%s: ldxi = %lld < m = %lld, or ldg = %lld or lda = %lld < n = %lld", me, (long long)ldxi, (long long)m, (long long)ldg,
                (long long)lda, (long long)n);
  mi_ctx_s *c = field->ctx;
  return guarded([&]() -> int {
    c->use();
    auto blocks = [&](const double *xi, int64_t ldx, double *g, int64_t lg, double *a, int64_t la) {
      for (int64_t r0 = 0; r0 < nreal; r0 += KLF_RB)
        field->launch_set((int)std::min<int64_t>(KLF_RB, nreal - r0), xi + (size_t)r0 * ldx, ldx, g ? g + (size_t)r0 * lg : nullptr, lg,
                          a ? a + (size_t)r0 * la : nullptr, la);
    };
    if (c->ptr_mode == MI_PTR_DEVICE) { blocks(Xi, ldxi, G, ldg, A, lda); return MI_OK; }
    hipStream_t s = c->stream;
    const size_t row = sizeof(double);
    DevBuf<double> dXi((size_t)m * nreal), dG, dA;
    MI_HIP(hipMemcpy2DAsync(dXi.p, row * m, Xi, row * ldxi, row * m, (size_t)nreal, hipMemcpyHostToDevice, s));
    if (G) dG.alloc((size_t)n * nreal);
    if (A) dA.alloc((size_t)n * nreal);
    blocks(dXi.p, m, G ? dG.p : nullptr, n, A ? dA.p : nullptr, n);
    if (G) MI_HIP(hipMemcpy2DAsync(G, row * ldg, dG.p, row * n, row * n, (size_t)nreal, hipMemcpyDeviceToHost, s));
    if (A) MI_HIP(hipMemcpy2DAsync(A, row * lda, dA.p, row * n, row * n, (size_t)nreal, hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    return MI_OK;
  });
}

int mi_kl_field_coords(mi_kl_field_t field, mi_op_t M, const double *g, double *xi) {
  const char *me = "mi_kl_field_coords";
  if (!field || !M || !M->impl || !g || !xi) return fail(MI_ERR_BAD_ARG, "%s: field, M, g or xi is NULL", me);
  if (field->dd) return fail(MI_ERR_BAD_ARG, "%s: coordinates are not provided for the factored form (no Psi is kept)", me);
  if (field->m > KLF_COORD_MAX_M) return fail(MI_ERR_BAD_ARG, "%s: m = %d modes (at most %lld for the coordinates)", me, field->m, (long long)KLF_COORD_MAX_M);
  CsrDev *csr = M->impl->as_csr();
  if (!csr || csr->n_rows != field->n || csr->n_cols != field->n || M->impl->ctx != field->ctx)
    return fail(MI_ERR_BAD_ARG, "%s: M is not a %d x %d sparse matrix (mi_csr_create) of the field's context", me, field->n, field->n);
  for (size_t a = 0; a < field->lam.size(); ++a)
    if (field->lam[a] == 0.0) return fail(MI_ERR_BAD_ARG, "%s: Lambda[%lld] = 0: the coordinate divides by sqrt(Lambda)", me, (long long)a);
  mi_ctx_s *c = field->ctx;
  return guarded([&]() -> int {
    c->use();
    if (c->ptr_mode == MI_PTR_DEVICE) { field->launch_coords(*csr, g, xi); return MI_OK; }
    DevBuf<double> gs, xs;
    In gi(c, g, (size_t)field->n, gs);
    InOut xo(c, xi, (size_t)field->m, xs, false);
    field->launch_coords(*csr, gi.dev, xo.dev);
    xo.finish();
    return MI_OK;
  });
}

int mi_kl_field_stats(mi_kl_field_t field, int64_t *bytes_kept, int64_t *bytes_per_set) {
  if (!field) return fail(MI_ERR_BAD_ARG, "mi_kl_field_stats: field is NULL");
  if (bytes_kept) *bytes_kept = field->bytes_kept;
  if (bytes_per_set) *bytes_per_set = field->bytes_per_set;
  return MI_OK;
}

int mi_kl_field_destroy(mi_kl_field_t field) {
  if (!field) return MI_OK;
  return guarded([&]() -> int {
    field->ctx->use();
    (void)hipStreamSynchronize(field->ctx->stream);
    delete field;
    return MI_OK;
  });
}

// ---------------------------------------------------------------- vector quantization of ξ (vq.hpp)
int mi_vq_tiling(int64_t d, int64_t ns, int64_t P, int64_t *point_tile, int64_t *cent_tile, int64_t *k_chunk, int64_t *cent_splits,
                 int64_t *sum_chunk) {
  if (d < 1 || ns < 1 || P < 1 || ns >= VQ_MAX_N || P >= VQ_MAX_N)
    return fail(MI_ERR_BAD_ARG, "mi_vq_tiling: d = %lld, ns = %lld, P = %lld: each at least 1, ns and P below 2^31", (long long)d, (long long)ns, (long long)P);
  if (point_tile) *point_tile = VQ_POINT_TILE;
  if (cent_tile) *cent_tile = VQ_CENT_TILE;
  if (k_chunk) *k_chunk = VQ_K_CHUNK;
  if (cent_splits) *cent_splits = vq_tiling(d, ns, P).splits;
  if (sum_chunk) *sum_chunk = VQ_SUM_CHUNK;
  return MI_OK;
}

// the checks every mi_vq_* call shares; MI_OK or the refusal (mi_last_error is set)
static int vq_check(const char *me, mi_ctx_t ctx, int64_t d, int64_t ns, const void *X, int64_t ldx, int64_t P, const void *C, int64_t ldc,
                    bool p_le_ns) {
  if (!ctx || !X || !C) return fail(MI_ERR_BAD_ARG, "%s: ctx, X or C is NULL", me);
  if (d < 1 || ns < 1 || P < 1 || ns >= VQ_MAX_N || P >= VQ_MAX_N || d >= VQ_MAX_N)
    return fail(MI_ERR_BAD_ARG, "%s: d = %lld, ns = %lld, P = %lld: each at least 1 and below 2^31", me, (long long)d, (long long)ns, (long long)P);
  if (p_le_ns && P > ns) return fail(MI_ERR_BAD_ARG, "%s: P = %lld centres for ns = %lld samples", me, (long long)P, (long long)ns);
  if (ldx < d || ldc < d) return fail(MI_ERR_BAD_ARG, "%s: ldx = %lld or ldc = %lld < d = %lld", me, (long long)ldx, (long long)ldc, (long long)d);
  if (ctx->has_comm()) return fail(MI_ERR_BAD_ARG, "%s: the context is one rank of several; sharded quantizers are not provided", me);
  return MI_OK;
}

int mi_vq_assign(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const double *C, int64_t ldc, int64_t *assign,
                 double *dist2, double *objv) {
  const char *me = "mi_vq_assign";
  if (int rc = vq_check(me, ctx, d, ns, X, ldx, P, C, ldc, false)) return rc;
  return guarded([&]() -> int {
    ctx->use();
    hipStream_t s = ctx->stream;
    VqArg<const double> x(ctx, X, (size_t)d, (size_t)ns, ldx, true), c(ctx, C, (size_t)d, (size_t)P, ldc, true);
    VqArg<long long> a(ctx, (long long *)assign, (size_t)ns, 1, ns, false);
    VqArg<double> d2(ctx, dist2, (size_t)ns, 1, ns, false);
    DevBuf<double> own;
    double *dd = d2.dev;
    if (!dd && objv) { own.alloc((size_t)ns); dd = own.p; }
    VqWork w(d, ns, P);
    w.assign(s, x.dev, x.ld, P, c.dev, c.ld, a.dev, dd, nullptr);
    if (objv) w.ordered_sum(s, dd, nullptr, nullptr);
    a.finish(); d2.finish();
    const double total = objv ? w.read_total(s) : 0.0;
    MI_HIP(hipStreamSynchronize(s));
    if (objv) *objv = total;
    return MI_OK;
  });
}

int mi_vq_update(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const int64_t *assign, double *C, int64_t ldc,
                 int64_t *counts) {
  const char *me = "mi_vq_update";
  if (int rc = vq_check(me, ctx, d, ns, X, ldx, P, C, ldc, false)) return rc;
  if (!assign || !counts) return fail(MI_ERR_BAD_ARG, "%s: assign or counts is NULL", me);
  return guarded([&]() -> int {
    ctx->use();
    hipStream_t s = ctx->stream;
    VqArg<const double> x(ctx, X, (size_t)d, (size_t)ns, ldx, true);
    VqArg<const long long> a(ctx, (const long long *)assign, (size_t)ns, 1, ns, true);
    if (ctx->ptr_mode != MI_PTR_DEVICE)   // refused before anything is written
      for (int64_t i = 0; i < ns; ++i)
        if (assign[i] < 0 || assign[i] >= P) return fail(MI_ERR_BAD_ARG, "%s: assign[%lld] = %lld outside [0, %lld)", me, (long long)i, (long long)assign[i], (long long)P);
    VqArg<double> c(ctx, C, (size_t)d, (size_t)P, ldc, true);
    VqArg<long long> n(ctx, (long long *)counts, (size_t)P, 1, P, false);
    VqWork w(d, ns, P);
    if (!w.update(s, x.dev, x.ld, a.dev, c.dev, c.ld, n.dev, true)) return fail(MI_ERR_BAD_ARG, "%s: an assignment outside [0, %lld)", me, (long long)P);
    c.finish(); n.finish();
    MI_HIP(hipStreamSynchronize(s));
    return MI_OK;
  });
}

int mi_vq_seed(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, const double *u, int64_t *picked, double *C,
               int64_t ldc) {
  const char *me = "mi_vq_seed";
  if (int rc = vq_check(me, ctx, d, ns, X, ldx, P, C, ldc, true)) return rc;
  if (!u || !picked) return fail(MI_ERR_BAD_ARG, "%s: u or picked is NULL", me);
  return guarded([&]() -> int {
    ctx->use();
    hipStream_t s = ctx->stream;
    VqArg<const double> x(ctx, X, (size_t)d, (size_t)ns, ldx, true), uu(ctx, u, (size_t)P, 1, P, true);
    // the centres are built in a buffer of the call's own, so that a refusal leaves C as it was
    DevBuf<double> cs((size_t)d * (size_t)P);
    DevBuf<long long> ps((size_t)P);
    VqWork w(d, ns, P);
    w.seed(s, x.dev, x.ld, uu.dev, ps.p, cs.p, d);
    if (w.read_err(s)) return fail(MI_ERR_BAD_ARG, "%s: the distances to the centres chosen so far sum to 0 (or are not finite): fewer distinct points than centres", me);
    const hipMemcpyKind kind = ctx->ptr_mode == MI_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    MI_HIP(hipMemcpy2DAsync(C, sizeof(double) * (size_t)ldc, cs.p, sizeof(double) * (size_t)d, sizeof(double) * (size_t)d, (size_t)P, kind, s));
    MI_HIP(hipMemcpyAsync(picked, ps.p, sizeof(long long) * (size_t)P, kind, s));
    MI_HIP(hipStreamSynchronize(s));
    return MI_OK;
  });
}

int mi_vq_kmeans(mi_ctx_t ctx, int64_t d, int64_t ns, const double *X, int64_t ldx, int64_t P, double *C, int64_t ldc, double tol,
                 int64_t maxiter, int64_t *assign, int64_t *counts, double *dist2, double *objv, int64_t *iters, int *converged) {
  const char *me = "mi_vq_kmeans";
  if (int rc = vq_check(me, ctx, d, ns, X, ldx, P, C, ldc, true)) return rc;
  if (!(tol >= 0.0) || !std::isfinite(tol) || maxiter < 0) return fail(MI_ERR_BAD_ARG, "%s: tol = %g, maxiter = %lld", me, tol, (long long)maxiter);
  return guarded([&]() -> int {
    ctx->use();
    hipStream_t s = ctx->stream;
    VqArg<const double> x(ctx, X, (size_t)d, (size_t)ns, ldx, true);
    VqArg<double> c(ctx, C, (size_t)d, (size_t)P, ldc, true);
    VqArg<long long> a(ctx, (long long *)assign, (size_t)ns, 1, ns, false), n(ctx, (long long *)counts, (size_t)P, 1, P, false);
    VqArg<double> d2(ctx, dist2, (size_t)ns, 1, ns, false);
    DevBuf<long long> own_a, own_n;
    DevBuf<double> own_d;
    long long *ad = a.dev, *nd = n.dev;
    double *dd = d2.dev;
    if (!ad) { own_a.alloc((size_t)ns); ad = own_a.p; }
    if (!nd) { own_n.alloc((size_t)P); nd = own_n.p; }
    if (!dd) { own_d.alloc((size_t)ns); dd = own_d.p; }
    VqWork w(d, ns, P);
    w.assign(s, x.dev, x.ld, P, c.dev, c.ld, ad, dd, nullptr);
    w.ordered_sum(s, dd, nullptr, nullptr);
    double obj = w.read_total(s);
    if (!std::isfinite(obj)) return fail(MI_ERR_BAD_ARG, "%s: the objective after the first assignment is %g (X or C is not finite)", me, obj);
    MI_HIP(hipMemsetAsync(nd, 0, (size_t)P * sizeof(long long), s));   // maxiter == 0: no update ever counts
    int64_t t = 0;
    bool conv = false;
    while (!conv && t < maxiter) {
      ++t;
      w.update(s, x.dev, x.ld, ad, c.dev, c.ld, nd, false);
      w.assign(s, x.dev, x.ld, P, c.dev, c.ld, ad, dd, nullptr);
      w.ordered_sum(s, dd, nullptr, nullptr);
      const double prev = obj;
      obj = w.read_total(s);
      conv = std::fabs(obj - prev) < tol;
    }
    c.finish(); a.finish(); n.finish(); d2.finish();
    MI_HIP(hipStreamSynchronize(s));
    if (objv) *objv = obj;
    if (iters) *iters = t;
    if (converged) *converged = conv ? 1 : 0;
    return MI_OK;
  });
}

// ---------------------------------------------------------------- z = Σ_i c_i (Π_i \ r) (vq.hpp)
static CombineOp *as_combine(mi_op_t op) { return op && op->impl ? dynamic_cast<CombineOp *>(op->impl.get()) : nullptr; }
static int combine_coef_check(const char *me, int64_t k, const double *coef) {
  if (!coef) return fail(MI_ERR_BAD_ARG, "%s: coef is NULL", me);
  for (int64_t i = 0; i < k; ++i)
    if (!std::isfinite(coef[i])) return fail(MI_ERR_BAD_ARG, "%s: coef[%lld] = %g is not finite", me, (long long)i, coef[i]);
  return MI_OK;
}
int mi_op_combine(mi_ctx_t ctx, int64_t k, const mi_op_t *ops, const double *coef, mi_op_t *op) {
  const char *me = "mi_op_combine";
  if (!ctx || !op) return fail(MI_ERR_BAD_ARG, "%s: ctx/op is NULL", me);
  *op = nullptr;
  if (k < 1 || k > 16) return fail(MI_ERR_BAD_ARG, "%s: k = %lld operators (1 <= k <= 16)", me, (long long)k);
  if (!ops) return fail(MI_ERR_BAD_ARG, "%s: ops is NULL", me);
  if (int rc = combine_coef_check(me, k, coef)) return rc;
  std::vector<mi_op_s *> kids;
  for (int64_t i = 0; i < k; ++i) {
    if (!ops[i] || !ops[i]->impl) return fail(MI_ERR_BAD_ARG, "%s: ops[%lld] is NULL", me, (long long)i);
    Operator *o = ops[i]->impl.get();
    if (dynamic_cast<AmgBankOp *>(o)) return fail(MI_ERR_BAD_ARG, "%s: ops[%lld] is an AMG bank, which is not applicable itself; combine views of it (mi_amg_bank_view)", me, (long long)i);
    if (dynamic_cast<CsrBatchOp *>(o)) return fail(MI_ERR_BAD_ARG, "%s: ops[%lld] is a batch of sparse matrices (mi_csr_batch_create), which is not applicable itself", me, (long long)i);
    if (o->ctx != ctx) return fail(MI_ERR_BAD_ARG, "%s: ops[%lld] belongs to another context", me, (long long)i);
    if (o->n != ops[0]->impl->n) return fail(MI_ERR_BAD_ARG, "%s: ops[%lld] is of size %lld, ops[0] of size %lld", me, (long long)i, (long long)o->n, (long long)ops[0]->impl->n);
    kids.push_back(ops[i]);
  }
  const int64_t n = kids[0]->impl->n;
  MI_NEW_OP(ctx, op, new CombineOp(ctx, n, kids, coef));
}
int mi_op_combine_set_coefficients(mi_op_t op, const double *coef) {
  const char *me = "mi_op_combine_set_coefficients";
  CombineOp *c = as_combine(op);
  if (!c) return fail(MI_ERR_BAD_ARG, "%s: not a combined operator", me);
  if (int rc = combine_coef_check(me, (int64_t)c->kids.size(), coef)) return rc;
  return guarded([&]() -> int {
    c->ctx->use();
    c->set_coefficients(coef);
    return MI_OK;
  });
}

// ---------------------------------------------------------------- P hierarchies on one plan (amg_bank.hpp)
static AmgBankOp *as_amg_bank(mi_op_t op) { return op && op->impl ? dynamic_cast<AmgBankOp *>(op->impl.get()) : nullptr; }
static AmgBankView *as_amg_bank_view(mi_op_t op) { return op && op->impl ? dynamic_cast<AmgBankView *>(op->impl.get()) : nullptr; }
static const char *bank_kind(mi_op_t op) {
  return !op || !op->impl ? "a NULL handle" : as_amg_bank(op) ? "an AMG bank" : as_amg_bank_view(op) ? "a view of an AMG bank" : "another kind of operator";
}
static int bank_member_check(const char *me, AmgBankOp *m, int64_t member, bool need_set) {
  if (member < 0 || member >= m->capacity)
    return fail(MI_ERR_BAD_ARG, "%s: member = %lld outside 0 .. %lld (the capacity is %lld)", me, (long long)member, (long long)m->capacity - 1, (long long)m->capacity);
  if (need_set && !m->is_set[(size_t)member])
    return fail(MI_ERR_BAD_ARG, "%s: member %lld was never set (mi_amg_bank_set_values)", me, (long long)member);
  return MI_OK;
}
int mi_amg_bank_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, int64_t nlevels, const int64_t *n_l,
                       const int64_t *const *agg, int64_t capacity, int index_base, mi_op_t *bank) {
  if (bank) *bank = nullptr;
  if (capacity < 1) return fail(MI_ERR_BAD_ARG, "mi_amg_bank_create: capacity = %lld (at least 1 member)", (long long)capacity);
  MI_NEW_OP(ctx, bank, new AmgBankOp(ctx, n, rowptr, colidx, nlevels, n_l, agg, capacity, index_base));
}
int mi_amg_bank_set_values(mi_op_t bank, int64_t member, const double *val) {
  const char *me = "mi_amg_bank_set_values";
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not an AMG bank (mi_amg_bank_create) but %s", me, bank_kind(bank));
  if (int rc = bank_member_check(me, m, member, false)) return rc;
  if (!val) return fail(MI_ERR_BAD_ARG, "%s: val is NULL", me);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    In vi(c, val, (size_t)m->eng.nnz0, m->eng.stage);
    m->set_values(member, vi.dev);   // synchronous
    return MI_OK;
  });
}
int mi_amg_bank_view(mi_op_t bank, int64_t max_terms, mi_op_t *view) {
  const char *me = "mi_amg_bank_view";
  if (view) *view = nullptr;
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not an AMG bank (mi_amg_bank_create) but %s", me, bank_kind(bank));
  if (max_terms < 1 || max_terms > AMGB_MAX_TERMS)
    return fail(MI_ERR_BAD_ARG, "%s: max_terms = %lld (1 <= max_terms <= %d)", me, (long long)max_terms, AMGB_MAX_TERMS);
  mi_ctx_s *ctx = m->ctx;
  MI_NEW_OP(ctx, view, new AmgBankView(ctx, m, (int)max_terms));
}
int mi_amg_bank_select(mi_op_t view, int64_t k, const int64_t *members, const double *coef) {
  const char *me = "mi_amg_bank_select";
  AmgBankView *v = as_amg_bank_view(view);
  if (!v) return fail(MI_ERR_BAD_ARG, "%s: not a view of an AMG bank (mi_amg_bank_view) but %s", me, bank_kind(view));
  if (k < 1 || k > v->kmax) return fail(MI_ERR_BAD_ARG, "%s: k = %lld members (1 <= k <= max_terms = %d)", me, (long long)k, v->kmax);
  if (!members) return fail(MI_ERR_BAD_ARG, "%s: members is NULL", me);
  if (int rc = combine_coef_check(me, k, coef)) return rc;
  for (int64_t i = 0; i < k; ++i)
    if (int rc = bank_member_check(me, v->bank, members[i], true)) return rc;
  return guarded([&]() -> int {
    v->ctx->use();
    v->write_selection(k, members, coef);
    return MI_OK;
  });
}
int mi_amg_bank_stats(mi_op_t bank, int64_t *capacity, int64_t *members_set, int64_t *bytes_shared, int64_t *bytes_per_member, int64_t *views) {
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_amg_bank_stats: not an AMG bank (mi_amg_bank_create) but %s", bank_kind(bank));
  if (capacity) *capacity = m->capacity;
  if (members_set) *members_set = m->n_set;
  if (bytes_shared) *bytes_shared = m->eng.kept + m->bws.bytes();   // (the batched set-up's workspace from its first call on)
  if (bytes_per_member) *bytes_per_member = 8 * m->stride;
  if (views) *views = m->views;
  return MI_OK;
}
int mi_amg_bank_level_sizes(mi_op_t bank, int64_t level, int64_t *n_rows, int64_t *n_cols, int64_t *a_nnz, int64_t *p_nnz) {
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_amg_bank_level_sizes: not an AMG bank (mi_amg_bank_create) but %s", bank_kind(bank));
  if (level < 0 || level >= m->nlev) return fail(MI_ERR_BAD_ARG, "mi_amg_bank_level_sizes: level = %lld of %d levels", (long long)level, m->nlev);
  m->eng.level_sizes((int)level, n_rows, n_cols, a_nnz, p_nnz);
  return MI_OK;
}
int mi_amg_bank_level_get(mi_op_t bank, int64_t member, int64_t level, int64_t *a_rowptr, int64_t *a_colidx, double *a_val, int64_t *p_rowptr,
                          int64_t *p_colidx, double *p_val, double *omega, double *omega_over_d) {
  const char *me = "mi_amg_bank_level_get";
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not an AMG bank (mi_amg_bank_create) but %s", me, bank_kind(bank));
  if (int rc = bank_member_check(me, m, member, true)) return rc;
  if (level < 0 || level >= m->nlev) return fail(MI_ERR_BAD_ARG, "%s: level = %lld of %d levels", me, (long long)level, m->nlev);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    m->level_get(member, (int)level, a_rowptr, a_colidx, a_val, p_rowptr, p_colidx, p_val, omega, omega_over_d);
    return MI_OK;
  });
}
int mi_amg_bank_coarse_inverse(mi_op_t bank, int64_t member, double *coarse_inv) {
  const char *me = "mi_amg_bank_coarse_inverse";
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not an AMG bank (mi_amg_bank_create) but %s", me, bank_kind(bank));
  if (int rc = bank_member_check(me, m, member, true)) return rc;
  if (!coarse_inv) return fail(MI_ERR_BAD_ARG, "%s: coarse_inv is NULL", me);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    MI_HIP(hipMemcpyAsync(coarse_inv, m->slot(member) + m->off_z, sizeof(double) * (size_t)m->nc * m->nc, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}

// ---------------------------------------------------------------- on-device block assembly
int mi_assembly_plan_create(mi_ctx_t ctx, int64_t nel, int64_t n_node, const int64_t *cells, int index_base, const double *G,
                            const double *area, const double *ue, const double *be, int64_t n_entries,
                            int64_t n_matrix_entries, const int64_t *cptr, const int64_t *ccode, mi_plan_t *plan) {
  if (!plan) return fail(MI_ERR_BAD_ARG, "plan is NULL");
  *plan = nullptr;
  if (!ctx || nel < 0 || n_node < 0 || n_entries < 0 || n_matrix_entries < 0 || n_matrix_entries > n_entries || !cptr ||
      (nel && (!cells || !G || !area || !ue || !be)) || (index_base != 0 && index_base != 1))
    return fail(MI_ERR_BAD_ARG, "mi_assembly_plan_create: bad argument");
  if (12 * nel >= INT32_MAX) return fail(MI_ERR_BAD_ARG, "mi_assembly_plan_create: 12*nel must fit 32 bits");
  return guarded([&]() -> int {
    ctx->use();
    const int64_t nc = cptr[n_entries];
    if (cptr[0] != 0 || nc < 0 || (nc && !ccode)) return fail(MI_ERR_BAD_ARG, "mi_assembly_plan_create: bad cptr / ccode");
    std::vector<long long> cp((size_t)n_entries + 1);
    for (int64_t k = 0; k <= n_entries; ++k) {
      if (cptr[k] < 0 || cptr[k] > nc || (k && cptr[k] < cptr[k - 1])) return fail(MI_ERR_BAD_ARG, "cptr is not monotone");
      cp[k] = cptr[k];
    }
    std::vector<int> cc((size_t)nc), cl((size_t)3 * nel);
    for (int64_t c = 0; c < nc; ++c) {
      if (ccode[c] < 0 || ccode[c] >= 12 * nel) return fail(MI_ERR_BAD_ARG, "contribution code %lld out of range", (long long)ccode[c]);
      cc[c] = (int)ccode[c];
    }
    for (int64_t k = 0; k < 3 * nel; ++k) cl[k] = to_i32(cells[k] - index_base, 0, n_node, "cells");
    std::unique_ptr<mi_plan_s> p(new mi_plan_s);
    p->ctx = ctx; p->nel = (int)nel; p->n_node = n_node; p->n_entries = n_entries; p->n_matrix = n_matrix_entries; p->n_contrib = nc;
    hipStream_t s = ctx->stream;
    p->cells.upload(cl, s); p->ccode.upload(cc, s); p->cptr.upload(cp, s);
    p->G.upload(G, (size_t)9 * nel, s); p->area.upload(area, (size_t)nel, s);
    p->ue.upload(ue, (size_t)3 * nel, s); p->be.upload(be, (size_t)3 * nel, s);
    p->da.alloc((size_t)nel + 1);
    MI_HIP(hipStreamSynchronize(s));
    *plan = p.release();
    return MI_OK;
  });
}
int mi_assembly_run(mi_plan_t plan, const double *a_nodal, double *values) {
  if (!plan || !a_nodal || (plan->n_entries && !values)) return fail(MI_ERR_BAD_ARG, "mi_assembly_run: NULL argument");
  if (plan->full) return fail(MI_ERR_BAD_ARG, "mi_assembly_run: this is a plan of mi_full_assembly_plan_create; mi_full_assembly_run executes it");
  mi_ctx_s *c = plan->ctx;
  return guarded([&]() -> int {
    c->use();
    In ai(c, a_nodal, (size_t)plan->n_node, plan->a_stage);
    InOut vo(c, values, (size_t)plan->n_entries, plan->out_stage, false);
    auto grid = [](int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + NT - 1) / NT, 1 << 20)); };
    if (plan->nel)
      hipLaunchKernelGGL(k_elem_coeff, dim3(grid(plan->nel)), dim3(NT), 0, c->stream, plan->nel, plan->cells.p, ai.dev, plan->da.p);
    if (plan->n_entries)
      hipLaunchKernelGGL(k_assemble_plan, dim3(grid(plan->n_entries)), dim3(NT), 0, c->stream, (long long)plan->n_entries,
                         (long long)plan->n_matrix, plan->nel, plan->cptr.p, plan->ccode.p, plan->da.p, plan->G.p, plan->area.p,
                         plan->ue.p, plan->be.p, vo.dev);
    MI_HIP(hipGetLastError());
    vo.finish();
    return MI_OK;
  });
}
int mi_assembly_plan_destroy(mi_plan_t plan) {
  if (!plan) return MI_OK;
  return guarded([&]() -> int {
    plan->ctx->use();
    (void)hipStreamSynchronize(plan->ctx->stream);
    delete plan;
    return MI_OK;
  });
}
// ---------------------------------------------------------------- on-device full-system assembly
int mi_full_assembly_plan_create(mi_ctx_t ctx, int64_t nel, int64_t n_node, const int64_t *cells, int index_base, const double *points,
                                 const int64_t *point_marker, int64_t n, const int64_t *rowptr, const int64_t *colidx, const double *ue,
                                 const double *be, mi_plan_t *plan) {
  const char *me = "mi_full_assembly_plan_create";
  if (!plan) return fail(MI_ERR_BAD_ARG, "%s: plan is NULL", me);
  *plan = nullptr;
  if (!ctx || !rowptr || !colidx || !ue || !be) return fail(MI_ERR_BAD_ARG, "%s: ctx, rowptr, colidx, ue or be is NULL", me);
  return guarded([&]() -> int {
    fap::Plan pl;
    std::string err;
    if (fap::make_plan(nel, n_node, cells, index_base, points, point_marker, n, rowptr, colidx, pl, err) != fap::OK)
      return fail(MI_ERR_BAD_ARG, "%s: %s", me, err.c_str());
    ctx->use();
    std::unique_ptr<mi_plan_s> p(new mi_plan_s);
    p->ctx = ctx; p->full = true; p->nel = pl.nel; p->n_node = pl.n_node; p->n = pl.n; p->nblk = pl.nblk();
    p->nnz = pl.nnz(); p->ninc = pl.ninc(); p->bytes_kept = pl.bytes();
    hipStream_t s = ctx->stream;
    p->cells.upload(pl.cells, s); p->rowptr.upload(pl.rowptr, s); p->diag_pos.upload(pl.diag_pos, s); p->inc_ptr.upload(pl.inc_ptr, s);
    p->inc_code.upload(pl.inc_code, s); p->inc_pos.upload(pl.inc_pos, s); p->blk_row.upload(pl.blk_row, s);
    p->points.upload(points, (size_t)2 * pl.n_node, s); p->ue.upload(ue, (size_t)3 * pl.nel, s); p->be.upload(be, (size_t)3 * pl.nel, s);
    MI_HIP(hipStreamSynchronize(s));
    p->rowptr_h.swap(pl.rowptr); p->colidx_h.swap(pl.colidx);
    *plan = p.release();
    return MI_OK;
  });
}
// values_dev, b_dev: device pointers
static void full_assembly_launch(mi_plan_s *p, const double *a_dev, double *values_dev, double *b_dev) {
  if (!p->nblk) return;
  const int per = (p->nblk + 7) / 8;
  hipLaunchKernelGGL(k_assemble_full, dim3(8 * per), dim3(FA_ROWS), 0, p->ctx->stream, p->nblk, per, p->nel, (int)p->n_node, p->blk_row.p,
                     p->rowptr.p, p->diag_pos.p, p->inc_ptr.p, p->inc_code.p, p->inc_pos.p, p->cells.p, p->points.p, p->ue.p, p->be.p,
                     a_dev, values_dev, b_dev);
  MI_HIP(hipGetLastError());
}
int mi_full_assembly_run(mi_plan_t plan, const double *a_nodal, double *values, double *b) {
  const char *me = "mi_full_assembly_run";
  if (!plan || !a_nodal) return fail(MI_ERR_BAD_ARG, "%s: NULL argument", me);
  if (!plan->full) return fail(MI_ERR_BAD_ARG, "%s: this is a plan of mi_assembly_plan_create; mi_assembly_run executes it", me);
  if ((plan->nnz && !values) || (plan->n && !b)) return fail(MI_ERR_BAD_ARG, "%s: values or b is NULL", me);
  mi_ctx_s *c = plan->ctx;
  return guarded([&]() -> int {
    c->use();
    In ai(c, a_nodal, (size_t)plan->n_node, plan->a_stage);
    InOut vo(c, values, (size_t)plan->nnz, plan->out_stage, false);
    InOut bo(c, b, (size_t)plan->n, plan->b_stage, false);
    full_assembly_launch(plan, ai.dev, vo.dev, bo.dev);
    vo.finish();
    bo.finish();
    return MI_OK;
  });
}
int mi_full_assembly_update(mi_plan_t plan, const double *a_nodal, mi_op_t A, double *b) {
  const char *me = "mi_full_assembly_update";
  if (!plan || !a_nodal) return fail(MI_ERR_BAD_ARG, "%s: NULL argument", me);
  if (!plan->full) return fail(MI_ERR_BAD_ARG, "%s: this is a plan of mi_assembly_plan_create", me);
  CsrOp *op = A && A->impl ? dynamic_cast<CsrOp *>(A->impl.get()) : nullptr;
  if (!op) return fail(MI_ERR_BAD_ARG, "%s: A is not a sparse matrix operator (mi_csr_create)", me);
  if (plan->n && !b) return fail(MI_ERR_BAD_ARG, "%s: b is NULL", me);
  mi_ctx_s *c = plan->ctx;
  if (op->ctx != c) return fail(MI_ERR_BAD_ARG, "%s: A belongs to another context", me);
  if (op->A.n_rows != plan->n || op->A.nnz != plan->nnz)
    return fail(MI_ERR_BAD_ARG, "%s: A is %d x %d with %lld stored entries, the plan's system %d x %d with %lld", me, op->A.n_rows, op->A.n_cols,
                (long long)op->A.nnz, plan->n, plan->n, (long long)plan->nnz);
  return guarded([&]() -> int {
    c->use();
    if (plan->checked_serial != op->serial) {   // once per operator: the whole pattern (synchronous)
      std::vector<int> rp((size_t)plan->n + 1), ci((size_t)plan->nnz);
      MI_HIP(hipMemcpyAsync(rp.data(), op->A.rowptr.p, rp.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      if (plan->nnz) MI_HIP(hipMemcpyAsync(ci.data(), op->A.col.p, ci.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      MI_HIP(hipStreamSynchronize(c->stream));
      if (rp != plan->rowptr_h || ci != plan->colidx_h) return fail(MI_ERR_BAD_ARG, "%s: the pattern of A is not the plan's", me);
      plan->checked_serial = op->serial;
    }
    In ai(c, a_nodal, (size_t)plan->n_node, plan->a_stage);
    InOut bo(c, b, (size_t)plan->n, plan->b_stage, false);
    full_assembly_launch(plan, ai.dev, op->A.val.p, bo.dev);
    bo.finish();
    return MI_OK;
  });
}
// ---------------------------------------------------------------- k matrices on one pattern, k solves in one loop (csr_batch.hpp, batch_solvers.hpp)
static CsrBatchOp *as_csr_batch(mi_op_t op) { return op && op->impl ? dynamic_cast<CsrBatchOp *>(op->impl.get()) : nullptr; }
static const char *batch_kind(mi_op_t op) {
  return !op || !op->impl ? "a NULL handle" : as_csr_batch(op) ? "a batch of sparse matrices" : bank_kind(op);
}
static int batch_slot_check(const char *me, CsrBatchOp *m, int64_t slot, bool need_set) {
  if (slot < 0 || slot >= m->capacity)
    return fail(MI_ERR_BAD_ARG, "%s: slot = %lld outside 0 .. %lld (the capacity is %lld)", me, (long long)slot, (long long)m->capacity - 1, (long long)m->capacity);
  if (need_set && !m->is_set[(size_t)slot])
    return fail(MI_ERR_BAD_ARG, "%s: slot %lld was never set (mi_csr_batch_set_values, mi_full_assembly_update_batch)", me, (long long)slot);
  return MI_OK;
}
int mi_csr_batch_create(mi_ctx_t ctx, int64_t n, const int64_t *rowptr, const int64_t *colidx, int64_t capacity, int index_base, mi_op_t *batch) {
  const char *me = "mi_csr_batch_create";
  if (batch) *batch = nullptr;
  if (!ctx || !batch) return fail(MI_ERR_BAD_ARG, "%s: ctx/batch is NULL", me);
  if (n < 1 || !rowptr || !colidx) return fail(MI_ERR_BAD_ARG, "%s: n = %lld (at least 1), rowptr or colidx is NULL", me, (long long)n);
  if (capacity < 1) return fail(MI_ERR_BAD_ARG, "%s: capacity = %lld (at least 1 slot)", me, (long long)capacity);
  if (index_base != 0 && index_base != 1) return fail(MI_ERR_BAD_ARG, "%s: index_base = %d (0 or 1)", me, index_base);
  return guarded([&]() -> int {
    ctx->use();
    const int64_t nnz = rowptr[n] - index_base;
    if (nnz < 0 || nnz >= INT32_MAX) raise(MI_ERR_BAD_ARG, "%s: bad rowptr[n]", me);
    std::vector<double> none((size_t)nnz, 0.0);
    HostCsr h = host_csr(n, n, rowptr, colidx, none.data(), index_base);
    std::unique_ptr<mi_op_s> hd(new mi_op_s);
    hd->impl.reset(new CsrBatchOp(ctx, h, capacity));
    MI_HIP(hipStreamSynchronize(ctx->stream));
    *batch = hd.release();
    return MI_OK;
  });
}
int mi_csr_batch_set_values(mi_op_t batch, int64_t slot, const double *val) {
  const char *me = "mi_csr_batch_set_values";
  CsrBatchOp *m = as_csr_batch(batch);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not a batch of sparse matrices (mi_csr_batch_create) but %s", me, batch_kind(batch));
  if (int rc = batch_slot_check(me, m, slot, false)) return rc;
  if (m->nnz && !val) return fail(MI_ERR_BAD_ARG, "%s: val is NULL", me);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    const bool dev = c->ptr_mode == MI_PTR_DEVICE;
    if (m->nnz) MI_HIP(hipMemcpyAsync(m->slot(slot), val, (size_t)m->nnz * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!dev) MI_HIP(hipStreamSynchronize(c->stream));   // the caller's array may change right after
    m->mark_set(slot);
    return MI_OK;
  });
}
int mi_csr_batch_get_values(mi_op_t batch, int64_t slot, double *val) {
  const char *me = "mi_csr_batch_get_values";
  CsrBatchOp *m = as_csr_batch(batch);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not a batch of sparse matrices (mi_csr_batch_create) but %s", me, batch_kind(batch));
  if (int rc = batch_slot_check(me, m, slot, true)) return rc;
  if (m->nnz && !val) return fail(MI_ERR_BAD_ARG, "%s: val is NULL", me);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    const bool dev = c->ptr_mode == MI_PTR_DEVICE;
    if (m->nnz) MI_HIP(hipMemcpyAsync(val, m->slot(slot), (size_t)m->nnz * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}
int mi_csr_batch_stats(mi_op_t batch, int64_t *capacity, int64_t *slots_set, int64_t *bytes_shared, int64_t *bytes_per_slot) {
  CsrBatchOp *m = as_csr_batch(batch);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_csr_batch_stats: not a batch of sparse matrices (mi_csr_batch_create) but %s", batch_kind(batch));
  if (capacity) *capacity = m->capacity;
  if (slots_set) *slots_set = m->n_set;
  if (bytes_shared) *bytes_shared = m->bytes_shared();
  if (bytes_per_slot) *bytes_per_slot = 8 * m->stride;
  return MI_OK;
}
int mi_csr_batch_stride(int64_t nnz, int64_t *doubles) {
  if (nnz < 0 || !doubles) return fail(MI_ERR_BAD_ARG, "mi_csr_batch_stride: nnz = %lld or doubles is NULL", (long long)nnz);
  *doubles = csr_batch_stride(nnz);
  return MI_OK;
}
int mi_full_assembly_update_batch(mi_plan_t plan, const double *a_nodal, mi_op_t batch, int64_t slot, double *b) {
  const char *me = "mi_full_assembly_update_batch";
  if (!plan || !a_nodal) return fail(MI_ERR_BAD_ARG, "%s: NULL argument", me);
  if (!plan->full) return fail(MI_ERR_BAD_ARG, "%s: this is a plan of mi_assembly_plan_create", me);
  CsrBatchOp *m = as_csr_batch(batch);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not a batch of sparse matrices (mi_csr_batch_create) but %s", me, batch_kind(batch));
  if (int rc = batch_slot_check(me, m, slot, false)) return rc;
  if (plan->n && !b) return fail(MI_ERR_BAD_ARG, "%s: b is NULL", me);
  mi_ctx_s *c = plan->ctx;
  if (m->ctx != c) return fail(MI_ERR_BAD_ARG, "%s: the batch belongs to another context", me);
  if (m->n != plan->n || m->nnz != plan->nnz)
    return fail(MI_ERR_BAD_ARG, "%s: the batch is %lld x %lld with %lld stored entries, the plan's system %d x %d with %lld", me, (long long)m->n, (long long)m->n,
                (long long)m->nnz, plan->n, plan->n, (long long)plan->nnz);
  return guarded([&]() -> int {
    c->use();
    if (plan->checked_serial != m->serial) {   // the first time this plan meets this batch: the whole pattern
      if (m->rowptr_h != plan->rowptr_h || m->col_h != plan->colidx_h) return fail(MI_ERR_BAD_ARG, "%s: the pattern of the batch is not the plan's", me);
      plan->checked_serial = m->serial;
    }
    In ai(c, a_nodal, (size_t)plan->n_node, plan->a_stage);
    InOut bo(c, b, (size_t)plan->n, plan->b_stage, false);
    full_assembly_launch(plan, ai.dev, m->slot(slot), bo.dev);
    bo.finish();
    m->mark_set(slot);
    return MI_OK;
  });
}
int mi_pcg_batch(mi_op_t A_batch, int64_t k, const int64_t *slots, mi_op_t M_view, const int64_t *members, const double *B, int64_t ldb, double *X,
                 int64_t ldx, int64_t maxit, double eps, double *res_norm, int64_t ldres, int64_t *it) {
  const char *me = "mi_pcg_batch";
  CsrBatchOp *a = as_csr_batch(A_batch);
  if (!a) return fail(MI_ERR_BAD_ARG, "%s: A is not a batch of sparse matrices (mi_csr_batch_create) but %s", me, batch_kind(A_batch));
  AmgBankView *v = nullptr;
  if (M_view) {
    v = as_amg_bank_view(M_view);
    if (!v) return fail(MI_ERR_BAD_ARG, "%s: M is not a view of an AMG bank (mi_amg_bank_view) but %s", me, batch_kind(M_view));
  }
  if (k < 1 || k > BATCH_MAX) return fail(MI_ERR_BAD_ARG, "%s: k = %lld systems (1 <= k <= %d)", me, (long long)k, BATCH_MAX);
  if (v && k > v->kmax) return fail(MI_ERR_BAD_ARG, "%s: k = %lld systems on a view of max_terms = %d", me, (long long)k, v->kmax);
  if (!slots || !B || !X || !it || (v && !members) || ldres < 0 || (ldres > 0 && !res_norm) || maxit < 0)
    return fail(MI_ERR_BAD_ARG, "%s: NULL or negative argument", me);
  mi_ctx_s *c = a->ctx;
  if (v && (v->n != a->n || v->ctx != c))
    return fail(MI_ERR_BAD_ARG, "%s: A and M differ in size or context (A is of size %lld, M of size %lld)", me, (long long)a->n, (long long)v->n);
  if (c->n_ranks > 1) return fail(MI_ERR_BAD_ARG, "%s: this context is rank %d of %d; a batched solve runs on a context of its own", me, c->rank, c->n_ranks);
  if (ldb < a->n || ldx < a->n) return fail(MI_ERR_BAD_ARG, "%s: ldb = %lld, ldx = %lld below n = %lld", me, (long long)ldb, (long long)ldx, (long long)a->n);
  for (int64_t t = 0; t < k; ++t) {
    if (int rc = batch_slot_check(me, a, slots[t], true)) return rc;
    if (v)
      if (int rc = bank_member_check(me, v->bank, members[t], true)) return rc;
  }
  return guarded([&]() -> int {
    c->use();
    const size_t n = (size_t)a->n;
    BatchKrylov kr(c, a, v);
    if (c->ptr_mode == MI_PTR_DEVICE) return kr.solve((int)k, slots, members, B, ldb, X, ldx, maxit, eps, res_norm, ldres, it);
    // Host pointers: the columns go through pinned buffers that the entry kernel reads and the exit kernel writes
    c->pin_b.ensure(n * (size_t)k); c->pin_x.ensure(n * (size_t)k);
    for (int64_t t = 0; t < k; ++t) {
      std::memcpy(c->pin_b.p + (size_t)t * n, B + (size_t)t * (size_t)ldb, n * sizeof(double));
      std::memcpy(c->pin_x.p + (size_t)t * n, X + (size_t)t * (size_t)ldx, n * sizeof(double));
    }
    const int rc = kr.solve((int)k, slots, members, c->pin_b.p, (int64_t)n, c->pin_x.p, (int64_t)n, maxit, eps, res_norm, ldres, it);  // synchronises before returning
    for (int64_t t = 0; t < k; ++t) std::memcpy(X + (size_t)t * (size_t)ldx, c->pin_x.p + (size_t)t * n, n * sizeof(double));
    return rc;
  });
}
int mi_amg_bank_set_values_batch(mi_op_t bank, int64_t k, const int64_t *members, mi_op_t A_batch, const int64_t *slots, int *status) {
  const char *me = "mi_amg_bank_set_values_batch";
  if (k < 1 || k > AMGB_MAX_TERMS) return fail(MI_ERR_BAD_ARG, "%s: k = %lld members (1 <= k <= %d)", me, (long long)k, AMGB_MAX_TERMS);
  AmgBankOp *m = as_amg_bank(bank);
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not an AMG bank (mi_amg_bank_create) but %s", me, batch_kind(bank));
  CsrBatchOp *a = as_csr_batch(A_batch);
  if (!a) return fail(MI_ERR_BAD_ARG, "%s: A is not a batch of sparse matrices (mi_csr_batch_create) but %s", me, batch_kind(A_batch));
  if (!members || !slots) return fail(MI_ERR_BAD_ARG, "%s: members or slots is NULL", me);
  mi_ctx_s *c = m->ctx;
  if (a->ctx != c) return fail(MI_ERR_BAD_ARG, "%s: the bank and the batch belong to different contexts", me);
  if (a->n != m->n || a->nnz != m->eng.nnz0)
    return fail(MI_ERR_BAD_ARG, "%s: the batch is %lld x %lld with %lld stored entries, the bank's matrix %lld x %lld with %lld", me, (long long)a->n,
                (long long)a->n, (long long)a->nnz, (long long)m->n, (long long)m->n, (long long)m->eng.nnz0);
  if (c->n_ranks > 1) return fail(MI_ERR_BAD_ARG, "%s: this context is rank %d of %d; a batched set-up runs on a context of its own", me, c->rank, c->n_ranks);
  for (int64_t t = 0; t < k; ++t) {
    if (int rc = bank_member_check(me, m, members[t], false)) return rc;
    if (int rc = batch_slot_check(me, a, slots[t], true)) return rc;
    for (int64_t u = 0; u < t; ++u)
      if (members[u] == members[t])
        return fail(MI_ERR_BAD_ARG, "%s: member %lld is given twice (terms %lld and %lld); a member is built once per call", me, (long long)members[t],
                    (long long)u, (long long)t);
  }
  if (m->batch_serial != a->serial) {   // the first time this bank meets this batch: the whole pattern
    const amgp::Level &H = m->eng.plan.lv[0];
    if (a->rowptr_h != H.a_ptr || a->col_h != H.a_col) return fail(MI_ERR_BAD_ARG, "%s: the pattern of the batch is not the bank's", me);
    m->batch_serial = a->serial;
  }
  return guarded([&]() -> int {
    c->use();
    std::vector<AsbTerm> term;
    m->set_values_batch((int)k, members, slots, a->slab.p, a->stride, term);   // synchronous
    std::string why;
    int bad = 0;
    for (int64_t t = 0; t < k; ++t) {
      const AsbTerm &T = term[(size_t)t];
      if (status) status[t] = T.ok ? MI_OK : MI_ERR_SINGULAR;
      if (T.ok) continue;
      char buf[400];
      std::snprintf(buf, sizeof buf, "%sterm %lld (member %lld, slot %lld): %s", bad ? "; " : "", (long long)t, (long long)members[t], (long long)slots[t],
                    T.why.c_str());
      why += buf;
      ++bad;
    }
    if (!bad) return MI_OK;
    const int rc = fail(MI_ERR_SINGULAR, "%s: %d of %lld terms failed; their members are kept as they were: %s", me, bad, (long long)k, why.c_str());
    return status ? MI_OK : rc;
  });
}
int mi_full_assembly_stats(mi_plan_t plan, int64_t *row_blocks, int64_t *incidences, int64_t *bytes_kept) {
  if (!plan || !plan->full) return fail(MI_ERR_BAD_ARG, "mi_full_assembly_stats: not a plan of mi_full_assembly_plan_create");
  if (row_blocks) *row_blocks = plan->nblk;
  if (incidences) *incidences = plan->ninc;
  if (bytes_kept) *bytes_kept = plan->bytes_kept;
  return MI_OK;
}
int mi_csr_set_values(mi_op_t op, const double *val) {
  const char *me = "mi_csr_set_values";
  CsrOp *m = op && op->impl ? dynamic_cast<CsrOp *>(op->impl.get()) : nullptr;
  if (!m) return fail(MI_ERR_BAD_ARG, "%s: not a sparse matrix operator (mi_csr_create)", me);
  if (m->A.nnz && !val) return fail(MI_ERR_BAD_ARG, "%s: val is NULL", me);
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    if (!m->A.nnz) return MI_OK;
    const bool dev = c->ptr_mode == MI_PTR_DEVICE;
    MI_HIP(hipMemcpyAsync(m->A.val.p, val, (size_t)m->A.nnz * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!dev) MI_HIP(hipStreamSynchronize(c->stream));   // the caller's array may change right after
    return MI_OK;
  });
}
int mi_diag_set_from_csr(mi_op_t M, mi_op_t A) {
  const char *me = "mi_diag_set_from_csr";
  DiagOp *d = M && M->impl ? dynamic_cast<DiagOp *>(M->impl.get()) : nullptr;
  CsrOp *a = A && A->impl ? dynamic_cast<CsrOp *>(A->impl.get()) : nullptr;
  if (!d || d->identity) return fail(MI_ERR_BAD_ARG, "%s: M is not a diagonal operator with values (mi_diag_create with dinv)", me);
  if (!a) return fail(MI_ERR_BAD_ARG, "%s: A is not a sparse matrix operator (mi_csr_create)", me);
  if (a->ctx != d->ctx) return fail(MI_ERR_BAD_ARG, "%s: M and A belong to different contexts", me);
  if (a->n != d->n) return fail(MI_ERR_BAD_ARG, "%s: M is of size %lld, A of size %lld", me, (long long)d->n, (long long)a->n);
  mi_ctx_s *c = d->ctx;
  return guarded([&]() -> int {
    c->use();
    if (!d->n) return MI_OK;
    DevBuf<int> flag(1);
    int missing = -1;
    MI_HIP(hipMemcpyAsync(flag.p, &missing, sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int grid = grid_for(d->n);
    hipLaunchKernelGGL(k_diag_from_csr, dim3(grid), dim3(NT), 0, c->stream, (int)d->n, 0, a->A.rowptr.p, a->A.col.p, a->A.val.p, d->dinv.p, flag.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(&missing, flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    if (missing >= 0) return fail(MI_ERR_BAD_ARG, "%s: row %d of A stores no diagonal entry", me, missing);
    hipLaunchKernelGGL(k_diag_from_csr, dim3(grid), dim3(NT), 0, c->stream, (int)d->n, 1, a->A.rowptr.p, a->A.col.p, a->A.val.p, d->dinv.p, flag.p);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(c->stream));   // `flag` goes back to the pool
    return MI_OK;
  });
}
static MatfreeSchurOp *as_matfree(mi_op_t op) {
  return op && op->impl ? dynamic_cast<MatfreeSchurOp *>(op->impl.get()) : nullptr;
}
int mi_schur_matfree_set_values(mi_op_t op, const double *ii_val, const double *ig_val, const double *gg_val) {
  MatfreeSchurOp *m = as_matfree(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_schur_matfree_set_values: not a matrix-free local-Schur operator");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> s1, s2, s3;
    In a(c, ii_val, ii_val && m->interior.cg() ? (size_t)m->interior.cg()->A.nnz : 0, s1), b(c, ig_val, ig_val ? (size_t)m->A_GI.nnz : 0, s2),
        g(c, gg_val, gg_val ? (size_t)m->A_GG.nnz : 0, s3);
    m->set_values(ii_val ? a.dev : nullptr, ig_val ? b.dev : nullptr, gg_val ? g.dev : nullptr);
    MI_HIP(hipStreamSynchronize(c->stream));  // staging buffers go out of scope
    return MI_OK;
  });
}
// either matrix-free Schur operator (MatfreeSchurOp, GlobalSchurOp): what the entry points below need is in their common base
static InteriorSchurOp *as_interior_schur(mi_op_t op) {
  return op && op->impl ? dynamic_cast<InteriorSchurOp *>(op->impl.get()) : nullptr;
}
static InteriorCg *interior_cg_of(mi_op_t op) {
  InteriorSchurOp *m = as_interior_schur(op);
  return m ? m->interior.cg() : nullptr;
}
int mi_schur_interior_precond(mi_op_t op, int kind) {
  InteriorCg *icg = interior_cg_of(op);
  if (!icg) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_precond: not a Schur operator with the interior solve on the device");
  if (kind != 0 && kind != 1) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_precond: kind must be 0 (none) or 1 (diagonal)");
  return guarded([&]() -> int {
    op->impl->ctx->use();
    icg->select(kind == 1 ? ICG_PL_DIAG : ICG_PL_NONE);
    return MI_OK;
  });
}
int mi_schur_interior_amg(mi_op_t op, int64_t nlevels, const int64_t *n_l, const int64_t *const *agg, int index_base) {
  InteriorCg *icg = interior_cg_of(op);
  if (!icg) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_amg: not a Schur operator with the interior solve on the device");
  if (as_interior_schur(op)->sharded()) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_amg: a sharded operator (the hierarchy is built on one device only)");
  mi_ctx_s *c = op->impl->ctx;
  return guarded([&]() -> int {
    c->use();
    interior_amg_select(c, *icg, nlevels, n_l, agg, index_base);
    return MI_OK;
  });
}
int mi_schur_interior_amg_stats(mi_op_t op, int64_t *levels, int64_t *coarse_n, int64_t *bytes_kept) {
  InteriorCg *icg = interior_cg_of(op);
  InteriorAmgStats st{};
  if (!icg || !interior_amg_stats(*icg, &st)) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_amg_stats: no AMG `Pl` is selected on this operator");
  if (levels) *levels = st.levels;
  if (coarse_n) *coarse_n = st.coarse_n;
  if (bytes_kept) *bytes_kept = st.bytes_kept;
  return MI_OK;
}
int mi_schur_interior_iterations(mi_op_t op, int64_t *iterations) {
  InteriorCg *icg = interior_cg_of(op);
  if (!icg || !iterations) return fail(MI_ERR_BAD_ARG, "mi_schur_interior_iterations: not a Schur operator with the interior solve on the device");
  *iterations = icg->total_iterations;
  return MI_OK;
}
int mi_schur_matfree_rhs(mi_op_t op, const double *b_I, const double *b_gamma, double *b_schur) {
  InteriorSchurOp *m = as_interior_schur(op);
  const int64_t ni_tot = m ? m->interior.ni_tot : 0;
  if (!m || !b_gamma || !b_schur || (ni_tot && !b_I))
    return fail(MI_ERR_BAD_ARG, "mi_schur_matfree_rhs: not a matrix-free (local or global) Schur operator, or NULL argument");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> s1;
    In bi(c, b_I, (size_t)ni_tot, s1), bg(c, b_gamma, (size_t)m->n, c->scratch_a);
    InOut out(c, b_schur, (size_t)m->n, c->scratch_b, false);
    m->schur_rhs(bi.dev, bg.dev, out.dev);
    out.finish();
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}

int mi_schur_matfree_interior_solutions(mi_op_t op, const double *u_gamma, const double *b_I, double *u_I) {
  InteriorSchurOp *m = as_interior_schur(op);
  const int64_t ni_tot = m ? m->interior.ni_tot : 0;
  if (!m || !u_gamma || (ni_tot && (!b_I || !u_I)))
    return fail(MI_ERR_BAD_ARG, "mi_schur_matfree_interior_solutions: not a matrix-free (local or global) Schur operator, or NULL argument");
  mi_ctx_s *c = m->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> s1, s2;
    In ug(c, u_gamma, (size_t)m->n, c->scratch_a), bi(c, b_I, (size_t)ni_tot, s1);
    InOut out(c, u_I, (size_t)ni_tot, s2, false);
    m->interior_solutions(ug.dev, bi.dev, out.dev);
    out.finish();
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}

// ---------------------------------------------------------------- set-up of the assembled mode on the device
int mi_schur_setup_create(mi_ctx_t ctx, int64_t ndom, const int64_t *n_gamma_d, const int64_t *n_i,
                          const int64_t *const *ii_colptr, const int64_t *const *ii_rowval, const int64_t *const *ig_colptr,
                          const int64_t *const *ig_rowval, const int64_t *const *gg_colptr, const int64_t *const *gg_rowval,
                          int index_base, mi_setup_t *plan) {
  if (!plan) return fail(MI_ERR_BAD_ARG, "plan is NULL");
  *plan = nullptr;
  if (!ctx || ndom <= 0 || !n_gamma_d || !n_i || !ii_colptr || !ii_rowval || !ig_colptr || !ig_rowval || !gg_colptr || !gg_rowval ||
      (index_base != 0 && index_base != 1))
    return fail(MI_ERR_BAD_ARG, "mi_schur_setup_create: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    std::unique_ptr<mi_setup_s> p(new mi_setup_s);
    setup_plan_build(*p, ctx, ndom, n_gamma_d, n_i, ii_colptr, ii_rowval, ig_colptr, ig_rowval, gg_colptr, gg_rowval, index_base);
    *plan = p.release();
    return MI_OK;
  });
}
int mi_schur_setup_run(mi_setup_t plan, const double *ii_val, const double *ig_val, const double *gg_val, const double *b_I,
                       double *Sd, double *w) {
  if (!plan || !ig_val || !gg_val || !Sd || (plan->n_ii && !ii_val)) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_run: NULL argument");
  mi_ctx_s *c = plan->ctx;
  return guarded([&]() -> int {
    c->use();
    In a(c, ii_val, (size_t)plan->n_ii, plan->st_ii), b(c, ig_val, (size_t)plan->n_ig, plan->st_ig), g(c, gg_val, (size_t)plan->n_gg, plan->st_gg),
        bi(c, b_I, b_I ? (size_t)plan->n_bi : 0, plan->st_bi);
    InOut so(c, Sd, (size_t)plan->n_s, plan->st_S, false), wo(c, w, w ? (size_t)plan->n_w : 0, plan->st_w, false);
    gj_run(*plan, a.dev, b.dev, g.dev, b_I ? bi.dev : nullptr, so.dev, w ? wo.dev : nullptr);
    so.finish();
    wo.finish();
    if (c->ptr_mode != MI_PTR_DEVICE) {   // host mode is synchronous: a break-down is reported
      // Gauss-Jordan elimination: no pivoting, so an interior block that is not positive definite shows as Inf / NaN
      // in S_d (the reference's CHOLMOD would throw PosDefException). Device-pointer mode stays asynchronous: there the
      // next mi_nn_pinv reports non-finite blocks.
      for (size_t i = 0; i < (size_t)plan->n_s; ++i)
        if (!std::isfinite(Sd[i])) return fail(MI_ERR_SINGULAR, "mi_schur_setup_run: S_d is not finite (an interior block is singular or not positive definite)");
    }
    return MI_OK;
  });
}
int mi_schur_setup_keep_levels(mi_setup_t plan, int on) {
  if (!plan) return fail(MI_ERR_BAD_ARG, "plan is NULL");
  if (!on && plan->bound > 0) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_keep_levels: %d live LORASC operator(s) solve with the kept levels", plan->bound);
  if (!on && plan->bound_nni > 0) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_keep_levels: %d live Neumann-Neumann induced operator(s) solve with the kept levels", plan->bound_nni);
  return guarded([&]() -> int {
    plan->ctx->use();
    gj_set_keep(*plan, on != 0);
    return MI_OK;
  });
}
int mi_schur_setup_interior_solve(mi_setup_t plan, const double *f, double *u) {
  if (!plan || !f || !u) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_interior_solve: NULL argument");
  mi_ctx_s *c = plan->ctx;
  return guarded([&]() -> int {
    c->use();
    DevBuf<double> s1, s2;
    In fi(c, f, (size_t)plan->n_bi, s1);
    InOut uo(c, u, (size_t)plan->n_bi, s2, false);
    gj_level_solve(*plan, fi.dev, uo.dev);
    uo.finish();
    if (c->ptr_mode != MI_PTR_DEVICE) MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
  });
}
int mi_schur_matfree_interior_levels(mi_op_t op, mi_setup_t plan) {
  if (!op || !op->impl) return fail(MI_ERR_BAD_ARG, "op is NULL");
  InteriorSchurOp *m = as_interior_schur(op);
  if (!m) return fail(MI_ERR_BAD_ARG, "mi_schur_matfree_interior_levels: not a matrix-free Schur operator");
  if (!plan) { m->interior.bind_levels(nullptr, nullptr); return MI_OK; }
  if (plan->ctx != m->ctx) return fail(MI_ERR_BAD_ARG, "plan and operator live on different contexts");
  const int ni_tot = m->interior.ni_tot, nd = m->interior.ndom();
  if ((long long)ni_tot != plan->n_bi || nd != plan->ndom)
    return fail(MI_ERR_BAD_ARG, "plan and operator differ in their subdomains (%d with %lld interior nodes vs %d with %lld)", plan->ndom, plan->n_bi, nd, (long long)ni_tot);
  return guarded([&]() -> int {
    // the plan counts the operator until it unbinds, binds another plan or is destroyed: mi_schur_setup_destroy waits for that
    m->interior.bind_levels([plan](const double *f, double *u) { gj_level_solve(*plan, f, u); }, &plan->bound_matfree);
    return MI_OK;
  });
}
int mi_schur_setup_destroy(mi_setup_t plan) {
  if (!plan) return MI_OK;
  if (plan->bound > 0) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_destroy: %d live LORASC operator(s) use this plan; destroy them first", plan->bound);
  if (plan->bound_nni > 0) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_destroy: %d live Neumann-Neumann induced operator(s) use this plan; destroy them first", plan->bound_nni);
  if (plan->bound_matfree > 0) return fail(MI_ERR_BAD_ARG, "mi_schur_setup_destroy: %d live matrix-free Schur operator(s) solve with this plan; destroy them first", plan->bound_matfree);
  return guarded([&]() -> int {
    plan->ctx->use();
    (void)hipStreamSynchronize(plan->ctx->stream);
    delete plan;
    return MI_OK;
  });
}
int mi_nn_pinv(mi_ctx_t ctx, int64_t ndom, const int64_t *n_gamma_d, const double *Sd, double rtol, double *PiSd) {
  if (!ctx || ndom <= 0 || !n_gamma_d || !Sd || !PiSd) return fail(MI_ERR_BAD_ARG, "mi_nn_pinv: bad argument");
  return guarded([&]() -> int {
    ctx->use();
    size_t tot = 0;
    for (int64_t d = 0; d < ndom; ++d) {
      if (n_gamma_d[d] < 0 || n_gamma_d[d] >= 46000) return fail(MI_ERR_BAD_ARG, "mi_nn_pinv: bad block size");
      tot += (size_t)n_gamma_d[d] * n_gamma_d[d];
    }
    if (rtol <= 0.0) rtol = std::sqrt(2.220446049250313e-16);   // sqrt(eps(Float64)), EPDD.jl:1211
    DevBuf<double> s1, s2;
    In si(ctx, Sd, tot, s1);
    InOut po(ctx, PiSd, tot, s2, false);
    pinv_blocks_fast(ctx, (int)ndom, n_gamma_d, si.dev, rtol, po.dev);
    po.finish();
    return MI_OK;
  });
}
static int dense_set_blocks(DenseBlockOp *dop, const double *blocks) {
  mi_ctx_s *c = dop->ctx;
  return guarded([&]() -> int {
    c->use();
    size_t tot = 0;
    for (int dl = 0; dl < dop->maps.ndl; ++dl) if (dop->owned_h[dl]) tot += (size_t)dop->maps.nd[dl] * dop->maps.nd[dl];
    if (dop->f32() && c->ptr_mode != MI_PTR_DEVICE) {   // as at creation: nothing fp32 cannot hold goes in silently
      size_t e = 0;
      for (int dl = 0; dl < dop->maps.ndl; ++dl) {
        if (!dop->owned_h[dl]) continue;
        const size_t nk = (size_t)dop->maps.nd[dl] * dop->maps.nd[dl];
        DenseBlockOp::check_f32_range(blocks + e, nk, dl);
        e += nk;
      }
    }
    DevBuf<double> st;
    In bi(c, blocks, tot, st);
    dop->set_blocks(bi.dev);
    if (c->ptr_mode != MI_PTR_DEVICE) MI_HIP(hipStreamSynchronize(c->stream));   // the staging buffer goes out of scope
    return MI_OK;
  });
}
int mi_dense_set_blocks(mi_op_t op, const double *blocks) {
  DenseBlockOp *dop = op && op->impl ? op->impl->as_dense() : nullptr;
  if (!dop || !blocks) return fail(MI_ERR_BAD_ARG, "mi_dense_set_blocks: not an assembled-Schur / Neumann-Neumann operator, or NULL blocks");
  return dense_set_blocks(dop, blocks);
}
int mi_nn_induced_set_blocks(mi_op_t op, const double *PiSd) {
  NnInducedOp *m = as_nn_induced(op);
  if (!m || !PiSd) return fail(MI_ERR_BAD_ARG, "mi_nn_induced_set_blocks: not a Neumann-Neumann induced preconditioner, or NULL PiSd");
  return dense_set_blocks(m->nn.get(), PiSd);
}

// ---------------------------------------------------------------- events
int mi_event_create(mi_event_t *ev) {
  if (!ev) return fail(MI_ERR_BAD_ARG, "ev is NULL");
  return guarded([&]() -> int {
    std::unique_ptr<mi_event_s> e(new mi_event_s);
    MI_HIP(hipEventCreate(&e->ev));
    *ev = e.release();
    return MI_OK;
  });
}
int mi_event_record(mi_ctx_t ctx, mi_event_t ev) {
  if (!ctx || !ev) return fail(MI_ERR_BAD_ARG, "NULL argument");
  return guarded([&]() -> int { ctx->use(); MI_HIP(hipEventRecord(ev->ev, ctx->stream)); return MI_OK; });
}
int mi_event_elapsed_ms(mi_event_t start, mi_event_t stop, double *ms) {
  if (!start || !stop || !ms) return fail(MI_ERR_BAD_ARG, "NULL argument");
  return guarded([&]() -> int {
    MI_HIP(hipEventSynchronize(stop->ev));
    float t = 0.f;
    MI_HIP(hipEventElapsedTime(&t, start->ev, stop->ev));
    *ms = (double)t;
    return MI_OK;
  });
}
int mi_event_destroy(mi_event_t ev) {
  if (!ev) return MI_OK;
  (void)hipEventDestroy(ev->ev);
  delete ev;
  return MI_OK;
}

}  // extern "C"
