// The level elimination of setup_plan.hpp on the device: kernels of this library only, batched over the subdomains and
// replayed from one hipGraph per realization (a chain of library BLAS-3 / LAPACK calls per level was measured and not
// adopted, profiles/NOTES.md: ~250 levels x dozens of small kernels per subdomain issued from the host, ~3 s per
// realization at config 3, bound by the host's launch rate; rocSOLVER cannot be captured into a graph).
//
// Formulation. With Z_k = T_k^{-1} kept explicitly (dense, symmetric) the recursion of setup_plan.hpp reads
//     T_k = A_kk - C_k' Z_{k+1} C_k,     g_k = b_k - C_k' (Z_{k+1} g_{k+1}),     Z_k = T_k^{-1},
//     S_d = A_ΓΓ - B' Z_0 B,             w_d = B' (Z_0 g_0),
// where C_k = A_{k+1,k} and B = A_IΓ[L_0, :] are SPARSE (a P1 node has <= 3-4 neighbours in the adjacent level), so every
// entry of C' Z C is a sum of a dozen picked entries of Z ("pick" kernels, one thread per entry) and the only dense
// O(n^3) work per level is the inversion of the SPD matrix T_k: an in-place-style block Gauss-Jordan inversion without
// pivoting (block size 64; the k-th pivot block of an SPD matrix is its k-th Schur complement, SPD again): the 64 x 64
// pivot block is inverted by one workgroup on the matrix cores — for the first block of a level in a launch of its own, for
// the others inside the previous step's update launch (look-ahead) —, and one launch per block step updates the whole
// matrix from the previous copy (ping-pong buffers: no launch reads what it writes) —
//     row panel   P A_Kj,   column panel   -A_iK P,   trailing   A_ij - A_iK (P A_Kj),   pivot block   P.
// All subdomains advance together (grid.z), aligned so that they reach level 0 in the same step. The launch sequence
// depends only on the plan: it is captured once and replayed per realization on plan-owned buffers.
#pragma once
#include <atomic>
#include <limits>

#include "operators.hpp"
#include "setup_plan.hpp"

namespace mi {

using SetupDom = setup::Dom;

constexpr int GJ_B = 64;    // pivot block: one full-matrix pass per 64 eliminated rows, its inverse by gj_invert_block64
constexpr int GJ_T = 64;    // tile of the update launch (256 threads, 4 x 4 outputs each)
constexpr int GJ_MAX_DOM = 65535;   // subdomains of one plan / blocks of one batch: they are the launches' grid.z
// LDS doubles behind the matrix a workgroup inverts. gj_invert_block64 uses 4 x 68 of them; the size is kept because it sets
// the update launch's footprint (50 KB, three workgroups per CU): shrinking it changes occupancy and needs its own measurement.
constexpr int GJ_SCRATCH = 32 * (GJ_T + 1) + 64;

struct GjStep {             // one per (step, subdomain); n0 == 0: the subdomain is not active in this step
  int n1, n0;               // size of the deeper level (dimension of Z_in; 0 at the subdomain's first step) and of this level
  int zin;                  // which ping-pong buffer holds Z_in (0 / 1)
  int cptr;                 // offset of C_k's column pointers (n0 + 1 entries)
  long long d_e0, d_e1;     // entry list of A_kk
  int b_off;                // offset of this level's nodes in `perm` (gather of b_k)
  int nb;                   // GJ block steps of this level = ceil(n0 / GJ_B)
  // level solves (the inverses Z_k kept after a run): where this level's Z lives in `zstore`, and the ROW form of the
  // coupling block C = A_{this level, next shallower level} (rows = this level's nodes) for the back-substitution
  long long zoff;
  int rptr;
};
struct GjDom {              // per subdomain
  double *T, *Z[2], *y, *g[2], *P;
  int ng, n_last, zfin;     // n_Γd; size of level 0; buffer holding Z_0
  int bptr;                 // offset of B's column pointers (ng + 1 entries)
  long long g_e0, g_e1;     // entry list of A_ΓΓ
  long long s_off, w_off;
  int nlev;
};

struct GjState {
  int nsteps = 0, ndom = 0, nmax = 0, ngmax = 0;
  std::vector<GjStep> steps_h;
  std::vector<GjDom> dom_h;
  std::vector<int> nb_step;          // GJ block steps to launch per step (max over the active subdomains)
  std::vector<int> n_step;           // largest level of the step (grid sizes)
  DevBuf<GjStep> steps;
  DevBuf<GjDom> doms;
  DevBuf<double> pool;               // all work buffers
  DevBuf<double> in_ii, in_ig, in_gg, in_bi, out_S, out_w;   // plan-owned I/O of the captured graph
  hipGraphExec_t graph[2] = {nullptr, nullptr};               // without / with right-hand side
  bool graph_failed = false;
  // level solves: A_IIdd \ f for all subdomains by forward / backward sweeps over the kept level inverses
  bool keep = false;
  DevBuf<double> zstore, gstore, ustore, sv_in, sv_out;
  DevBuf<int> r_ptr, r_col, r_src;
  hipGraphExec_t solve_graph = nullptr;
  bool have_levels = false;                                   // a run with keep == true has filled zstore
  ~GjState() {
    for (auto &g : graph) if (g) (void)hipGraphExecDestroy(g);
    if (solve_graph) (void)hipGraphExecDestroy(solve_graph);
  }
};
}  // namespace mi

// The plan of mi_schur_setup_create: the host plan, its arrays on the device, and the state of the elimination
struct mi_setup_s : mi::setup::Plan {
  mi_ctx_s *ctx = nullptr;
  mi::DevBuf<int> src, dst, perm;        // entry lists of A_kk and A_ΓΓ of all subdomains; interior permutation (concatenated)
  mi::DevBuf<int> c_ptr, c_row, c_src;   // column form of the coupling blocks
  mi::DevBuf<double> st_ii, st_ig, st_gg, st_bi, st_S, st_w;   // staging for host-pointer calls
  std::unique_ptr<mi::GjState> gj;       // block Gauss-Jordan elimination, batched over the subdomains, replayed from a hipGraph
  int bound = 0;                         // operators that borrow this plan (lorasc.hpp): mi_schur_setup_destroy is refused while > 0
  int bound_nni = 0;                     // ... and the Neumann-Neumann induced operators that do (nn_induced.hpp)
  int bound_matfree = 0;                 // ... and the matrix-free Schur operators that solve their interiors with its levels (InteriorSolver)
};

namespace mi {

inline void setup_plan_build(mi_setup_s &P, mi_ctx_s *c, int64_t ndom, const int64_t *n_gamma_d, const int64_t *n_i,
                             const int64_t *const *ii_ptr, const int64_t *const *ii_idx, const int64_t *const *ig_ptr,
                             const int64_t *const *ig_idx, const int64_t *const *gg_ptr, const int64_t *const *gg_idx, int base) {
  setup::Input in;
  in.ndom = ndom; in.base = base; in.n_gamma_d = n_gamma_d; in.n_i = n_i;
  in.ii_ptr = ii_ptr; in.ii_idx = ii_idx; in.ig_ptr = ig_ptr; in.ig_idx = ig_idx; in.gg_ptr = gg_ptr; in.gg_idx = gg_idx;
  std::string err;
  if (setup::make_plan(in, P, err) != setup::OK) raise(MI_ERR_BAD_ARG, "%s", err.c_str());
  P.ctx = c;
  hipStream_t s = c->stream;
  P.src.upload(P.src_h, s); P.dst.upload(P.dst_h, s); P.perm.upload(P.perm_h, s);
  P.c_ptr.upload(P.c_ptr_h, s); P.c_row.upload(P.c_row_h, s); P.c_src.upload(P.c_src_h, s);
  for (auto *v : {&P.src_h, &P.dst_h, &P.perm_h}) std::vector<int>().swap(*v);   // read on the device only; the column form keeps its host copy (row_form)
}

#pragma clang fp contract(fast)

// (a runtime index into an array member of a by-value struct sends the whole struct to scratch memory: 120 bytes per thread
// in every kernel below; a select keeps it in scalar registers)
#define GJ_Z(dm, k) ((k) ? (dm).Z[1] : (dm).Z[0])
#define GJ_G(dm, k) ((k) ? (dm).g[1] : (dm).g[0])

// T[i,j] = -(C' Z C)[i,j]  (0 at a subdomain's first step); the entries of A_kk are added by k_gj_scatter.
// One thread per entry of the UPPER triangle (the mirror image is stored with it: C' Z C is symmetric, and the two
// summation orders differ in the last bit only). A column of C holds a handful of entries (a P1 node has <= 3-4
// neighbours in the adjacent level): up to PK of them are fetched into registers first, so that all picked entries of Z
// are requested together instead of one dependent chain per entry; longer columns take the plain loops.
__global__ __launch_bounds__(256) void k_gj_pick(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                 const int *__restrict__ c_ptr, const int *__restrict__ c_row,
                                                 const int *__restrict__ c_src, const double *__restrict__ ii_val) {
  constexpr int PK = 4;
  if (blockIdx.y < blockIdx.x) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  const int n0 = st.n0;
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= n0 || j >= n0 || i > j) return;
  const GjDom dm = doms[blockIdx.z];
  double acc = 0.0;
  if (st.n1 > 0) {
    const double *Z = GJ_Z(dm, st.zin);
    const int *cp = c_ptr + st.cptr;
    const int ia = cp[i], ib = cp[i + 1], ja = cp[j], jb = cp[j + 1];
    const int na = ib - ia, nb = jb - ja;
    if (na <= PK && nb <= PK) {
      int ra[PK], rb[PK], sa[PK], sb[PK];
      double va[PK], vb[PK];
#pragma unroll
      for (int k = 0; k < PK; ++k) {
        ra[k] = k < na ? c_row[ia + k] : 0; sa[k] = k < na ? c_src[ia + k] : 0;
        rb[k] = k < nb ? c_row[ja + k] : 0; sb[k] = k < nb ? c_src[ja + k] : 0;
      }
#pragma unroll
      for (int k = 0; k < PK; ++k) { va[k] = k < na ? ii_val[sa[k]] : 0.0; vb[k] = k < nb ? ii_val[sb[k]] : 0.0; }
      double z[PK][PK];
#pragma unroll
      for (int p_ = 0; p_ < PK; ++p_)
#pragma unroll
        for (int q = 0; q < PK; ++q) z[p_][q] = (p_ < na && q < nb) ? Z[(size_t)ra[p_] + (size_t)rb[q] * st.n1] : 0.0;
#pragma unroll
      for (int p_ = 0; p_ < PK; ++p_)
        if (p_ < na) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < PK; ++q)
            if (q < nb) s += z[p_][q] * vb[q];
          acc += va[p_] * s;
        }
    } else {
      for (int p_ = ia; p_ < ib; ++p_) {
        const double ci = ii_val[c_src[p_]];
        const double *zr = Z + (size_t)c_row[p_];           // Z[a, :] read as Z[a + b*n1] (symmetric)
        double s = 0.0;
        for (int q = ja; q < jb; ++q) s += zr[(size_t)c_row[q] * st.n1] * ii_val[c_src[q]];
        acc += ci * s;
      }
    }
  }
  dm.T[i + (size_t)j * n0] = -acc;
  if (i != j) dm.T[j + (size_t)i * n0] = -acc;
}
__global__ __launch_bounds__(256) void k_gj_scatter(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                    const int *__restrict__ src, const int *__restrict__ dst,
                                                    const double *__restrict__ ii_val) {
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (st.n0 == 0) return;
  double *T = doms[blockIdx.z].T;
  for (long long e = st.d_e0 + blockIdx.x * 256ll + threadIdx.x; e < st.d_e1; e += (long long)gridDim.x * 256) T[dst[e]] += ii_val[src[e]];
}
// y = Z g for 64 rows per workgroup (Z symmetric, column-major: a wave reads 64 consecutive rows of one column); the
// columns are dealt to the four waves and the partial sums meet in LDS
__device__ __forceinline__ void gj_gemv64(const double *__restrict__ Z, int n, const double *__restrict__ g, double *__restrict__ y) {
  __shared__ double part[4][64];
  const int r = blockIdx.x * 64 + (threadIdx.x & 63), wv = threadIdx.x >> 6;
  double s = 0.0;
  if (r < n)
    for (int b0 = wv; b0 < n; b0 += 64) {      // sixteen columns in flight per thread (four: 0.4 TB/s — ~100 workgroups cannot fill the chip otherwise); same order of the sum
      double z[16], gg[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int b = b0 + 4 * k;
        z[k] = b < n ? Z[r + (size_t)b * n] : 0.0;
        gg[k] = b < n ? g[b] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) s += z[k] * gg[k];
    }
  part[wv][threadIdx.x & 63] = s;
  __syncthreads();
  if (threadIdx.x < 64 && r < n) y[r] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void k_gj_zg(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms) {
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (st.n0 == 0 || (int)blockIdx.x * 64 >= st.n1) return;
  const GjDom dm = doms[blockIdx.z];
  gj_gemv64(GJ_Z(dm, st.zin), st.n1, GJ_G(dm, (step + 1) & 1), dm.y);
}
// g_k = b_k - C_k' y
__global__ __launch_bounds__(256) void k_gj_g(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                              const int *__restrict__ c_ptr, const int *__restrict__ c_row, const int *__restrict__ c_src,
                                              const double *__restrict__ ii_val, const int *__restrict__ perm, const double *__restrict__ bI) {
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= st.n0) return;
  const GjDom dm = doms[blockIdx.z];
  double v = bI[perm[st.b_off + j]];
  if (st.n1 > 0) {
    const int *cp = c_ptr + st.cptr;
    double s = 0.0;
    for (int p = cp[j]; p < cp[j + 1]; ++p) s += ii_val[c_src[p]] * dm.y[c_row[p]];
    v -= s;
  }
  GJ_G(dm, step & 1)[j] = v;
}

// ---- block Gauss-Jordan inversion of T (n0 x n0, SPD), block step kb: source = T (kb == 0) or Z[kb & 1], destination Z[(kb + 1) & 1]
__device__ __forceinline__ const double *gj_src(const GjDom &dm, int kb) { return kb == 0 ? dm.T : GJ_Z(dm, kb & 1); }
typedef double gj_d4 __attribute__((ext_vector_type(4)));
// inverse of a 4 x 4 matrix (row-major m) whose leading 2 x 2 block and its Schur complement are non-singular (pivot blocks of
// an SPD matrix are): [A B; C D]^{-1} = [Ai + X Si V, -X Si; -Si V, Si],  Ai = A^{-1}, X = Ai B, V = C Ai, S = D - C X, Si = S^{-1}
__device__ __forceinline__ void gj_inv4(const double (&m)[16], double (&p)[16]) {
  const double da = 1.0 / (m[0] * m[5] - m[1] * m[4]);
  const double a00 = m[5] * da, a01 = -m[1] * da, a10 = -m[4] * da, a11 = m[0] * da;
  const double x00 = a00 * m[2] + a01 * m[6], x01 = a00 * m[3] + a01 * m[7], x10 = a10 * m[2] + a11 * m[6], x11 = a10 * m[3] + a11 * m[7];
  const double v00 = m[8] * a00 + m[9] * a10, v01 = m[8] * a01 + m[9] * a11, v10 = m[12] * a00 + m[13] * a10, v11 = m[12] * a01 + m[13] * a11;
  const double s00 = m[10] - (m[8] * x00 + m[9] * x10), s01 = m[11] - (m[8] * x01 + m[9] * x11);
  const double s10 = m[14] - (m[12] * x00 + m[13] * x10), s11 = m[15] - (m[12] * x01 + m[13] * x11);
  const double ds = 1.0 / (s00 * s11 - s01 * s10);
  const double i00 = s11 * ds, i01 = -s01 * ds, i10 = -s10 * ds, i11 = s00 * ds;
  const double y00 = x00 * i00 + x01 * i10, y01 = x00 * i01 + x01 * i11, y10 = x10 * i00 + x11 * i10, y11 = x10 * i01 + x11 * i11;   // X Si
  const double z00 = i00 * v00 + i01 * v10, z01 = i00 * v01 + i01 * v11, z10 = i10 * v00 + i11 * v10, z11 = i10 * v01 + i11 * v11;   // Si V
  p[0] = a00 + (x00 * z00 + x01 * z10); p[1] = a01 + (x00 * z01 + x01 * z11); p[2] = -y00; p[3] = -y01;
  p[4] = a10 + (x10 * z00 + x11 * z10); p[5] = a11 + (x10 * z01 + x11 * z11); p[6] = -y10; p[7] = -y11;
  p[8] = -z00; p[9] = -z01; p[10] = i00; p[11] = i01;
  p[12] = -z10; p[13] = -z11; p[14] = i10; p[15] = i11;
}
// In-place inverse of a 64 x 64 SPD block in LDS (row stride LD) by 256 threads: block Gauss-Jordan with 4 x 4 pivots —
// 16 block steps instead of 64 scalar ones. A step: every thread inverts the pivot block M[K, K] in registers (redundantly:
// no broadcast of the result needed); thread (k, j) forms one entry of the row panel R = P M[K, :] (columns K: P itself);
// then D = C - M[:, K] R is ONE 16 x 16 x 4 matrix-core op per 16 x 16 block (C = M, zero in columns K, so those become the
// column panel -M[:, K] P); rows K take R. Two barriers per step. `Rb`: 4 x 68 doubles of scratch. Beyond the matrix' end
// the caller puts the identity. The chain of these 16 steps is the serial part of every block step of the elimination
// (every tile of the next launch waits for it): 21 us per pivot block, 1.3 us per step, of which 0.7-0.9 are the four
// matrix-core ops with their operand moves; the tiles' LDS traffic is not what a step waits for (tools/probes/inv_probe.hip).
__device__ __forceinline__ void gj_invert_block64(double *M, int LD, double *Rb, bool mirror) {
  constexpr int RL = 68;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = l & 15, lk = l >> 4;
#pragma unroll 1
  for (int s = 0; s < 16; ++s) {
    const int k0 = 4 * s;
    double m[16], p[16];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) m[4 * a + b] = M[(k0 + a) * LD + k0 + b];
    gj_inv4(m, p);
    {
      double q0, q1, q2, q3;                       // row wv of P (wave-uniform choice)
      if (wv == 0) { q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3]; }
      else if (wv == 1) { q0 = p[4]; q1 = p[5]; q2 = p[6]; q3 = p[7]; }
      else if (wv == 2) { q0 = p[8]; q1 = p[9]; q2 = p[10]; q3 = p[11]; }
      else { q0 = p[12]; q1 = p[13]; q2 = p[14]; q3 = p[15]; }
      const int j = l, jj = j & 3;
      const bool inK = (j >> 2) == s;
      // (unconditional loads, then the choice: a load under `?:` becomes a branch with its own wait — four serial LDS round trips)
      const double w0 = M[(k0 + 0) * LD + j], w1 = M[(k0 + 1) * LD + j], w2 = M[(k0 + 2) * LD + j], w3 = M[(k0 + 3) * LD + j];
      const double v0 = inK ? (jj == 0 ? 1.0 : 0.0) : w0, v1 = inK ? (jj == 1 ? 1.0 : 0.0) : w1;
      const double v2 = inK ? (jj == 2 ? 1.0 : 0.0) : w2, v3 = inK ? (jj == 3 ? 1.0 : 0.0) : w3;
      Rb[wv * RL + j] = ((q0 * v0 + q1 * v1) + q2 * v2) + q3 * v3;
    }
    __syncthreads();
    const double aop = M[(16 * wv + lc) * LD + k0 + lk];        // M[row block wv][K]: A[row = lc][k = lk]
    const bool krows = wv == (s >> 2);
    const int vk = s & 3;
    double rb[4];
    gj_d4 d[4];
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) {                            // every operand first (one LDS round trip), then the matrix cores, then the stores
      const int col = 16 * bj + lc;
      rb[bj] = Rb[lk * RL + col];
#pragma unroll
      for (int v = 0; v < 4; ++v) d[bj][v] = M[(16 * wv + lk + 4 * v) * LD + col];
    }
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) {
      const bool cK = ((16 * bj + lc) >> 2) == s;
#pragma unroll
      for (int v = 0; v < 4; ++v) d[bj][v] = cK ? 0.0 : d[bj][v];
      d[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop, -rb[bj], d[bj], 0, 0, 0);
    }
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) {
      const int col = 16 * bj + lc;
#pragma unroll
      for (int v = 0; v < 4; ++v) M[(16 * wv + lk + 4 * v) * LD + col] = (krows && v == vk) ? rb[bj] : d[bj][v];   // row 16 wv + lk + 4 v is pivot row k0 + lk exactly then
    }
    __syncthreads();
  }
  // `mirror` (the block is the whole matrix, P the result): symmetric to the last bit, the upper triangle mirrored. NOT when
  // P feeds further block steps: the two triangles of an unpivoted Gauss-Jordan inverse carry errors of order κ eps that
  // cancel in the next Schur complement D - B' (P B) only as computed; with one triangle replaced by the other that
  // complement loses up to κ² eps (|Z - T^-1| / |T^-1| = 0.41 at κ = 1e8, n = 65, instead of 7e-5; the update kernels
  // read P[t][k] as stored, they do not assume it symmetric).
  if (!mirror) return;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (j > i) M[j * LD + i] = M[i * LD + j];
  }
  __syncthreads();
}
// The pivot inverse of block step kb lives in P + (kb & 1) * GJ_B^2: the update launch of step kb reads it while one of its
// workgroups writes the inverse for step kb + 1 into the other half (look-ahead, below). This kernel serves kb = 0 only.
__global__ __launch_bounds__(256) void k_gj_pivot(int step, int kb, int ndom, const GjStep *__restrict__ steps,
                                                  const GjDom *__restrict__ doms) {
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (kb >= st.nb) return;
  const GjDom dm = doms[blockIdx.z];
  const int n = st.n0, k0 = kb * GJ_B, bs = min(GJ_B, n - k0);
  const double *A = gj_src(dm, kb);
  constexpr int LD = GJ_B + 1;
  __shared__ double Mb[GJ_B * LD];
  __shared__ double Wb[GJ_SCRATCH];
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) {
    const int r = e % GJ_B, c = e / GJ_B;
    Mb[r * LD + c] = (r < bs && c < bs) ? A[(k0 + r) + (size_t)(k0 + c) * n] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  gj_invert_block64(Mb, LD, Wb, st.nb == 1);   // one pivot block: its inverse is the result, mirrored to symmetry
  double *Pd = dm.P + (kb & 1) * (GJ_B * GJ_B);
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) Pd[e] = Mb[(e % GJ_B) * LD + e / GJ_B];   // column-major GJ_B x GJ_B
}
// one 64 x 64 tile of the updated matrix from the previous copy, on the fp64 matrix cores (v_mfma_f64_16x16x4_f64:
// A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], D: col = l & 15, row = (l >> 4) + 4 reg). R = P A[K, J] (64 x 64) first, then
// the trailing update computed TRANSPOSED — the instruction's row index runs over the tile's columns j, its column index
// over the tile's rows i — so that a lane's four results sit in 16-lane groups of consecutive i: loads and stores of the
// column-major matrix are 128-byte segments. Wave v owns rows 16 v .. 16 v + 15 of the tile.
__global__ __launch_bounds__(256, 3) void k_gj_update(int step, int kb, int ndom, const GjStep *__restrict__ steps,
                                                   const GjDom *__restrict__ doms) {
  // a pivot block as wide as a tile: every lane keeps its share of A[I, K] in registers, and the tiles of block column K
  // are a zero-start product with P (both below)
  static_assert(GJ_B == GJ_T, "pivot block and tile have one width");
  const int dz = blockIdx.z, gbx = blockIdx.x, gby = blockIdx.y;
  const GjStep st = steps[(size_t)step * ndom + dz];
  const int n = st.n0;
  if (kb >= st.nb || gbx * GJ_T >= n || gby * GJ_T >= n) return;   // (the swap below stays inside the grid: td * GJ_T < n)
  const GjDom dm = doms[dz];
  const int k0 = kb * GJ_B, bs = min(GJ_B, n - k0);
  const double *A = gj_src(dm, kb);
  double *O = GJ_Z(dm, (kb + 1) & 1);
  // Look-ahead: the tile that holds the NEXT pivot block (diagonal tile td) also inverts it once it has updated it, so that
  // the next block step needs no pivot launch of its own (a serial chain of 21 us per step, 5 400 steps per
  // realization at config 3). That tile is dealt first (swapped with tile (0, 0)) so that its longer life stays inside the launch.
  const int k1 = k0 + GJ_B, td = k1 / GJ_T;
  const bool ahead = kb + 1 < st.nb;
  int bx = gbx, by = gby;
  if (ahead) {
    if (bx == 0 && by == 0) bx = by = td;
    else if (bx == td && by == td) bx = by = 0;
  }
  const bool special = ahead && bx == td && by == td;
  // SYMMETRY. With σ(i) = -1 for the indices already swept (i < k0) and +1 otherwise, the matrix between two block steps
  // satisfies M[j,i] = σ(i) σ(j) M[i,j] (the inverse pivot block and the trailing part are symmetric, the row panel P A_Kj
  // and the column panel -A_iK P are each other's negative transpose; induction over the steps, P symmetric). Only the
  // tiles on and above the diagonal are computed; an off-diagonal tile also writes its mirror image (transposed through
  // LDS so that both stores are 128-byte segments). Storage stays full: the pick kernels and the next step's panel loads
  // read any entry.
  if (bx > by) return;
  const int i0 = bx * GJ_T, j0 = by * GJ_T;
  // LDS: A[K, J] / R (GJ_B x 65) and the scratch of the look-ahead inversion: 50 KB per workgroup, THREE workgroups per CU
  // — the 530-620 tiles of a config-3 launch are resident at once instead of running a second round for the last few
  // (profiles/NOTES.md). Neither the pivot inverse P nor A[I, K] is staged: every lane keeps the GJ_B / 4 entries of each
  // that it feeds to the matrix cores in registers (P: one request per entry, served by L2: every tile reads the same 32 KB).
  constexpr int LDS_R = GJ_B * (GJ_T + 1);
  static_assert(LDS_R >= GJ_T * (GJ_T + 1), "the mirror image of a tile is staged in the R buffer");
  __shared__ double lds[LDS_R + GJ_SCRATCH];
  double (&R)[GJ_B][GJ_T + 1] = *reinterpret_cast<double (*)[GJ_B][GJ_T + 1]>(lds);           // A[K, J] first, then R = P * A[K, J], then (look-ahead tile) the next pivot block
  double (&Ak)[GJ_B][GJ_T + 1] = R;
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, lc = l & 15, lk = l >> 4;
  const double *Pcur = dm.P + (kb & 1) * (GJ_B * GJ_B);   // column-major, symmetric
  // R = P A[K, J]: 4 x 4 blocks of 16 x 16; wave wv owns t-block wv and all four j-blocks
  double pa[GJ_B / 4];                                                   // P[16 wv + lc][kk + lk], kk = 0, 4, ...
#pragma unroll
  for (int q = 0; q < GJ_B / 4; ++q) pa[q] = Pcur[(16 * wv + lc) + (size_t)(4 * q + lk) * GJ_B];
  for (int e = threadIdx.x; e < GJ_B * GJ_T; e += 256) {
    const int t = e % GJ_B, c = e / GJ_B;        // A[k0 + t, j0 + c]: consecutive threads walk down a column
    Ak[t][c] = (t < bs && j0 + c < n) ? A[(k0 + t) + (size_t)(j0 + c) * n] : 0.0;
  }
  double cb[GJ_B / 4];                           // A[i0 + 16 wv + lc, k0 + 4 q + lk]
  {
    const int ir = i0 + 16 * wv + lc;
#pragma unroll
    for (int q = 0; q < GJ_B / 4; ++q) cb[q] = (4 * q + lk < bs && ir < n) ? A[ir + (size_t)(k0 + 4 * q + lk) * n] : 0.0;
  }
  // the old entries this lane will update (D layout of the transposed product): i = i0 + 16 wv + lc, j = j0 + 16 jt + lk + 4 v
  const int i = i0 + 16 * wv + lc;
  gj_d4 acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + 16 * jt + lk + 4 * v;
      acc[jt][v] = (i < n && j < n) ? A[i + (size_t)j * n] : 0.0;
    }
  // The tiles of block column K (by == kb, above the diagonal) hold only column-panel entries -(A_iK P): the SAME
  // matrix-core loop as the trailing update with P in place of R and a zero start
  // (D[j][i] = Σ_u P[u][j] (-A[i][k0 + u])); the diagonal tile (kb, kb) becomes P itself.
  const bool kcol = by == kb;
  __syncthreads();
  if (!kcol) {
    gj_d4 d[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      d[q] = gj_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < GJ_B; kk += 4)
        d[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk / 4], Ak[kk + lk][16 * q + lc], d[q], 0, 0, 0);
    }
    __syncthreads();                             // every wave has read A[K, J]: the buffer becomes R
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int v = 0; v < 4; ++v) R[16 * wv + lk + 4 * v][16 * q + lc] = d[q][v];
    }
  } else {
    __syncthreads();
    for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256)    // P[u][jl] (columns beyond bs: identity, times a zero panel)
      R[e % GJ_B][e / GJ_B] = Pcur[e];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = gj_d4{0.0, 0.0, 0.0, 0.0};
  }
  __syncthreads();
  // acc[jt] (rows j, cols i) -= R[K, J_jt]' * A[I, K]'  ==  (A_ij - A_iK (P A_Kj))'
#pragma unroll
  for (int kk = 0; kk < GJ_B; kk += 4) {
    const double bneg = -cb[kk / 4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(R[kk + lk][16 * jt + lc], bneg, acc[jt], 0, 0, 0);
  }
  const bool ik = i >= k0 && i < k0 + bs;
  const int bs1 = min(GJ_B, n - k1);
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int jl = 16 * jt + lk + 4 * v, j = j0 + jl;
      if (i >= n || j >= n) continue;
      const bool jk = j >= k0 && j < k0 + bs;
      double val = acc[jt][v];                                                 // A_ij - A_iK (P A_Kj);  block column K: -(A_iK P)[i, j - k0]
      if (ik && jk) val = Pcur[(i - k0) + (size_t)(j - k0) * GJ_B];
      else if (ik) val = R[i - k0][jl];                                        // (P A_Kj)[i - k0, j]
      O[i + (size_t)j * n] = val;
      acc[jt][v] = val;
    }
  if (bx != by) {                                // the mirror image: M[j,i] = σ'(i) σ'(j) M[i,j], σ' = -1 below k1 (swept after this step)
    __syncthreads();                             // R is read for the last time above
    double *T = lds;                             // [GJ_T][GJ_T + 1]
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int jl = 16 * jt + lk + 4 * v, j = j0 + jl;
        const double sg = ((i < k1) != (j < k1)) ? -1.0 : 1.0;
        T[jl * (GJ_T + 1) + 16 * wv + lc] = sg * acc[jt][v];
      }
    __syncthreads();
    const int r = j0 + 16 * wv + lc;             // row of the mirror tile (a column index of this tile)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int cl = 16 * jt + lk + 4 * v, cg = i0 + cl;
        if (r < n && cg < n) O[r + (size_t)cg * n] = T[(16 * wv + lc) * (GJ_T + 1) + cl];
      }
    return;
  }
  if (!special) return;
  // Look-ahead: this diagonal tile holds the next pivot block (rows / columns k1 .. k1 + bs1 of the updated matrix); its inverse
  // goes to the other half of P. R becomes the landing zone (row stride GJ_T + 1), the rest of `lds` the inversion's scratch.
  __syncthreads();
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) { const int rr = e / GJ_B, cc = e % GJ_B; R[rr][cc] = rr == cc ? 1.0 : 0.0; }   // identity beyond the matrix' end
  __syncthreads();
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + 16 * jt + lk + 4 * v;
      if (i >= k1 && i < k1 + bs1 && j >= k1 && j < k1 + bs1) R[i - k1][j - k1] = acc[jt][v];   // (trailing entries: K1 != K)
    }
  __syncthreads();
  gj_invert_block64(&R[0][0], GJ_T + 1, lds + LDS_R, false);   // (block kb + 1 >= 1: P feeds further block steps, not mirrored)
  double *Pn = dm.P + ((kb + 1) & 1) * (GJ_B * GJ_B);
  for (int e = threadIdx.x; e < GJ_B * GJ_B; e += 256) Pn[e] = R[e % GJ_B][e / GJ_B];
}
// ---- the end of a subdomain's chain: S (upper triangle mirrored) = A_ΓΓ - B' Z_0 B; w = B' (Z_0 g_0)
__global__ __launch_bounds__(256) void k_gj_final_pick(int ndom, const GjDom *__restrict__ doms, const int *__restrict__ c_ptr,
                                                       const int *__restrict__ c_row, const int *__restrict__ c_src,
                                                       const double *__restrict__ ig_val) {
  const GjDom dm = doms[blockIdx.z];
  const int ng = dm.ng;
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= ng || j >= ng) return;
  double acc = 0.0;
  if (dm.n_last > 0) {
    const double *Z = GJ_Z(dm, dm.zfin);
    const int *cp = c_ptr + dm.bptr;
    for (int p = cp[i]; p < cp[i + 1]; ++p) {
      const double ci = ig_val[c_src[p]];
      const double *zr = Z + (size_t)c_row[p];
      double s = 0.0;
      for (int q = cp[j]; q < cp[j + 1]; ++q) s += zr[(size_t)c_row[q] * dm.n_last] * ig_val[c_src[q]];
      acc += ci * s;
    }
  }
  dm.T[i + (size_t)j * ng] = -acc;
}
__global__ __launch_bounds__(256) void k_gj_final_scatter(int ndom, const GjDom *__restrict__ doms, const int *__restrict__ src,
                                                          const int *__restrict__ dst, const double *__restrict__ gg_val) {
  const GjDom dm = doms[blockIdx.z];
  for (long long e = dm.g_e0 + blockIdx.x * 256ll + threadIdx.x; e < dm.g_e1; e += (long long)gridDim.x * 256) dm.T[dst[e]] += gg_val[src[e]];
}
__global__ __launch_bounds__(256) void k_gj_final_sym(int ndom, const GjDom *__restrict__ doms, double *__restrict__ Sd) {
  const GjDom dm = doms[blockIdx.z];
  const int ng = dm.ng;
  const long long tot = (long long)ng * ng;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) {
    const int i = (int)(e % ng), j = (int)(e / ng);
    Sd[dm.s_off + e] = i <= j ? dm.T[i + (size_t)j * ng] : dm.T[j + (size_t)i * ng];   // `Symmetric(Array(...))`, EPDD.jl:692
  }
}
__global__ __launch_bounds__(256) void k_gj_final_zg(int ndom, int last_step, const GjDom *__restrict__ doms) {
  const GjDom dm = doms[blockIdx.z];
  if ((int)blockIdx.x * 64 >= dm.n_last) return;
  gj_gemv64(GJ_Z(dm, dm.zfin), dm.n_last, GJ_G(dm, last_step & 1), dm.y);
}
__global__ __launch_bounds__(256) void k_gj_final_w(int ndom, const GjDom *__restrict__ doms, const int *__restrict__ c_ptr,
                                                    const int *__restrict__ c_row, const int *__restrict__ c_src,
                                                    const double *__restrict__ ig_val, double *__restrict__ w) {
  const GjDom dm = doms[blockIdx.z];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= dm.ng) return;
  double s = 0.0;
  if (dm.n_last > 0) {
    const int *cp = c_ptr + dm.bptr;
    for (int p = cp[j]; p < cp[j + 1]; ++p) s += ig_val[c_src[p]] * dm.y[c_row[p]];
  }
  w[dm.w_off + j] = s;
}
// ---- level solves. After a run with `keep`, zstore holds Z_k = T_k^{-1} of every level of every subdomain, and
//     A_IIdd \ f   =   forward:  g_m = f_m,  g_k = f_k - C_k' (Z_{k+1} g_{k+1})        (deepest level first: the run's own recursion)
//                      backward: u_0 = Z_0 g_0,  u_{k+1} = Z_{k+1} (g_{k+1} - C_k u_k)  (C_k = A_{k+1,k})
// is an EXACT interior solve (block LDL' over the breadth-first levels): two streams of the kept inverses instead of the
// thousands of A_II SpMVs of the reference's `IterativeSolvers.cg` (EPDD.jl:648-650).
__global__ __launch_bounds__(256) void k_gj_keep(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                 double *__restrict__ zstore) {
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (st.n0 == 0) return;
  const GjDom dm = doms[blockIdx.z];
  const double *src = GJ_Z(dm, st.nb & 1);
  double *dst = zstore + st.zoff;
  const long long tot = (long long)st.n0 * st.n0;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) dst[e] = src[e];
}
// y = Z_{k+1} g_{k+1} (the deeper level, handled one step earlier)
__global__ __launch_bounds__(256) void k_lv_zg(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                               const double *__restrict__ zstore, const double *__restrict__ gstore, const int *done) {
  if (done && *done) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (st.n0 == 0 || st.n1 == 0 || (int)blockIdx.x * 64 >= st.n1) return;
  const GjStep sp = steps[(size_t)(step - 1) * ndom + blockIdx.z];
  gj_gemv64(zstore + sp.zoff, st.n1, gstore + sp.b_off, doms[blockIdx.z].y);
}
// g_k = f_k - C_k' y  (f in the caller's interior order, g in level order)
__global__ __launch_bounds__(256) void k_lv_g(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                              const int *__restrict__ c_ptr, const int *__restrict__ c_row, const int *__restrict__ c_src,
                                              const double *__restrict__ ii_val, const int *__restrict__ perm, const double *__restrict__ f,
                                              double *__restrict__ gstore, const int *done) {
  if (done && *done) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= st.n0) return;
  double v = f[perm[st.b_off + j]];
  if (st.n1 > 0) {
    const double *y = doms[blockIdx.z].y;
    const int *cp = c_ptr + st.cptr;
    double s2 = 0.0;
    for (int p = cp[j]; p < cp[j + 1]; ++p) s2 += ii_val[c_src[p]] * y[c_row[p]];
    v -= s2;
  }
  gstore[st.b_off + j] = v;
}
// u = Z (g - C u_shallower) for the level of `step` (64 rows per workgroup; the operand is formed in LDS first: every
// workgroup needs all of it). last == 1: the shallowest level, u_0 = Z_0 g_0.
constexpr int LV_MAX = 2048;
// 64 rows per workgroup of out = Z t (Z n x n column-major, t in LDS): the columns dealt to the four waves, sixteen in flight
// per thread, the partial sums combined as (p0 + p1) + (p2 + p3). The one place that fixes the summation order of the
// back-substitution (k_lv_back) and of block_jacobi.hpp's Γ step and level 0.
__device__ __forceinline__ void lv_gemv64_lds(const double *__restrict__ Z, int n, const double *t, double (*part)[64], double *__restrict__ out) {
  const int r = blockIdx.x * 64 + (threadIdx.x & 63), wv = threadIdx.x >> 6;
  double s2 = 0.0;
  if (r < n)
    for (int b0 = wv; b0 < n; b0 += 64) {
      double z[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) { const int b = b0 + 4 * k; z[k] = b < n ? Z[r + (size_t)b * n] : 0.0; }
#pragma unroll
      for (int k = 0; k < 16; ++k) { const int b = b0 + 4 * k; if (b < n) s2 += z[k] * t[b]; }
    }
  part[wv][threadIdx.x & 63] = s2;
  __syncthreads();
  if (threadIdx.x < 64 && r < n) out[r] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void k_lv_back(int step, int last, int ndom, const GjStep *__restrict__ steps,
                                                 const double *__restrict__ zstore, const double *__restrict__ gstore,
                                                 const int *__restrict__ r_ptr, const int *__restrict__ r_col, const int *__restrict__ r_src,
                                                 const double *__restrict__ ii_val, double *__restrict__ ustore, const int *done) {
  if (done && *done) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  const int n = st.n0;
  if (n == 0 || (int)blockIdx.x * 64 >= n) return;
  __shared__ double t[LV_MAX];
  __shared__ double part[4][64];
  const double *g = gstore + st.b_off;
  if (last) {
    for (int i = threadIdx.x; i < n; i += 256) t[i] = g[i];
  } else {
    const GjStep sn = steps[(size_t)(step + 1) * ndom + blockIdx.z];      // the shallower level: its u is known
    const double *us = ustore + sn.b_off;
    const int *rp = r_ptr + st.rptr;
    for (int i = threadIdx.x; i < n; i += 256) {
      double s2 = 0.0;
      for (int p = rp[i]; p < rp[i + 1]; ++p) s2 += ii_val[r_src[p]] * us[r_col[p]];
      t[i] = g[i] - s2;
    }
  }
  __syncthreads();
  lv_gemv64_lds(zstore + st.zoff, n, t, part, ustore + st.b_off);
}
__global__ __launch_bounds__(256) void k_lv_scatter(long long n, const int *__restrict__ perm, const double *__restrict__ ustore, double *__restrict__ u) {
  for (long long q = blockIdx.x * 256ll + threadIdx.x; q < n; q += (long long)gridDim.x * 256) u[perm[q]] = ustore[q];
}
#pragma clang fp contract(off)

inline void gj_build(mi_setup_s &P) {
  std::unique_ptr<GjState> G(new GjState);
  G->ndom = P.ndom;
  int smax = 0;
  for (auto &D : P.dom) { smax = std::max(smax, D.nlev); G->nmax = std::max(G->nmax, D.max_lev); G->ngmax = std::max(G->ngmax, D.n_g); }
  G->nsteps = smax;
  G->steps_h.assign((size_t)std::max(1, smax) * P.ndom, GjStep{});
  G->nb_step.assign(std::max(1, smax), 0);
  G->n_step.assign(std::max(1, smax), 1);
  // work buffers: T also receives the final n_Γd x n_Γd pick
  size_t tot = 0;
  std::vector<size_t> off_T(P.ndom), off_Z0(P.ndom), off_Z1(P.ndom), off_y(P.ndom), off_g0(P.ndom), off_g1(P.ndom), off_P(P.ndom);
  for (int d = 0; d < P.ndom; ++d) {
    const SetupDom &D = P.dom[d];
    const size_t nm = (size_t)std::max(1, D.max_lev), nt = (size_t)std::max<int>(std::max(1, D.max_lev), D.n_g);
    auto take = [&](size_t cnt) { const size_t o = tot; tot += (cnt + 31) / 32 * 32; return o; };
    off_T[d] = take(nt * nt); off_Z0[d] = take(nm * nm); off_Z1[d] = take(nm * nm);
    off_y[d] = take(nm); off_g0[d] = take(nm); off_g1[d] = take(nm); off_P[d] = take(2 * GJ_B * GJ_B);
  }
  G->pool.alloc(tot + 32);
  memset_sync(G->pool.p, 0, sizeof(double) * (tot + 32));
  G->dom_h.resize(P.ndom);
  for (int d = 0; d < P.ndom; ++d) {
    const SetupDom &D = P.dom[d];
    GjDom &q = G->dom_h[d];
    q.T = G->pool.p + off_T[d]; q.Z[0] = G->pool.p + off_Z0[d]; q.Z[1] = G->pool.p + off_Z1[d];
    q.y = G->pool.p + off_y[d]; q.g[0] = G->pool.p + off_g0[d]; q.g[1] = G->pool.p + off_g1[d]; q.P = G->pool.p + off_P[d];
    q.ng = D.n_g; q.nlev = D.nlev; q.bptr = D.bptr_off; q.g_e0 = D.g_e0; q.g_e1 = D.g_e1; q.s_off = D.s_off; q.w_off = D.w_off;
    q.n_last = D.nlev ? D.lev_off[1] - D.lev_off[0] : 0;
    q.zfin = 0;
    int zin = 0;
    for (int k = D.nlev - 1; k >= 0; --k) {           // level k is handled in step smax - 1 - k
      const int step = smax - 1 - k;
      GjStep &st = G->steps_h[(size_t)step * P.ndom + d];
      st.n0 = D.lev_off[k + 1] - D.lev_off[k];
      st.n1 = k + 1 < D.nlev ? D.lev_off[k + 2] - D.lev_off[k + 1] : 0;
      st.zin = zin;
      st.cptr = k + 1 < D.nlev ? D.cptr_off[k] : 0;
      st.d_e0 = D.d_e0[k]; st.d_e1 = D.d_e0[k + 1];
      st.b_off = (int)D.bi_off + D.lev_off[k];
      st.nb = (st.n0 + GJ_B - 1) / GJ_B;
      zin = st.nb & 1;                                 // block step kb writes Z[(kb + 1) & 1]: the inverse ends in Z[nb & 1]
      G->nb_step[step] = std::max(G->nb_step[step], st.nb);
      G->n_step[step] = std::max(G->n_step[step], std::max(st.n0, st.n1));
    }
    q.zfin = zin;
  }
  hipStream_t s = P.ctx->stream;
  G->steps.upload(G->steps_h, s);
  G->doms.upload(G->dom_h, s);
  G->in_ii.alloc((size_t)P.n_ii + 1); G->in_ig.alloc((size_t)P.n_ig + 1); G->in_gg.alloc((size_t)P.n_gg + 1);
  G->in_bi.alloc((size_t)P.n_bi + 1); G->out_S.alloc((size_t)P.n_s + 1); G->out_w.alloc((size_t)P.n_w + 1);
  P.gj = std::move(G);
}

// The block steps of one level of `n` subdomains or blocks (grid.z), of which the longest takes nb_max steps and the widest
// has n_max rows: the first pivot block in a launch of its own, every later one by look-ahead inside the update launches.
inline void gj_block_steps(hipStream_t s, int step, int nb_max, int n_max, int n, const GjStep *steps, const GjDom *doms) {
  const int tx = (n_max + GJ_T - 1) / GJ_T;
  for (int kb = 0; kb < nb_max; ++kb) {
    if (kb == 0) hipLaunchKernelGGL(k_gj_pivot, dim3(1, 1, n), dim3(256), 0, s, step, kb, n, steps, doms);
    hipLaunchKernelGGL(k_gj_update, dim3(tx, tx, n), dim3(256), 0, s, step, kb, n, steps, doms);
  }
}

// enqueue the whole elimination on `s` (plain launches: capturable)
inline void gj_enqueue(mi_setup_s &P, hipStream_t s, const double *ii, const double *ig, const double *gg, const double *bI, double *Sd,
                       double *w) {
  GjState &G = *P.gj;
  const int nd = P.ndom;
  const GjStep *st = G.steps.p;
  const GjDom *dm = G.doms.p;
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  int nm = std::max(1, G.nmax);
  if (nd > GJ_MAX_DOM) raise(MI_ERR_BAD_ARG, "device set-up: more than %d subdomains in one plan", GJ_MAX_DOM);
  for (int step = 0; step < G.nsteps; ++step) {
    nm = G.n_step[step];   // grids cover the largest level of this step only
    if (bI && step > 0) hipLaunchKernelGGL(k_gj_zg, dim3(cdiv(nm, 64), 1, nd), dim3(256), 0, s, step, nd, st, dm);
    hipLaunchKernelGGL(k_gj_pick, dim3(cdiv(nm, 16), cdiv(nm, 16), nd), dim3(256), 0, s, step, nd, st, dm, P.c_ptr.p, P.c_row.p, P.c_src.p, ii);
    hipLaunchKernelGGL(k_gj_scatter, dim3(8, 1, nd), dim3(256), 0, s, step, nd, st, dm, P.src.p, P.dst.p, ii);
    if (bI) hipLaunchKernelGGL(k_gj_g, dim3(cdiv(nm, 256), 1, nd), dim3(256), 0, s, step, nd, st, dm, P.c_ptr.p, P.c_row.p, P.c_src.p, ii, P.perm.p, bI);
    gj_block_steps(s, step, G.nb_step[step], nm, nd, st, dm);
    if (G.keep) hipLaunchKernelGGL(k_gj_keep, dim3(std::min(1024, cdiv(nm * nm, 1024)), 1, nd), dim3(256), 0, s, step, nd, st, dm, G.zstore.p);
  }
  const int ngm = std::max(1, G.ngmax);
  nm = std::max(1, G.nmax);
  hipLaunchKernelGGL(k_gj_final_pick, dim3(cdiv(ngm, 16), cdiv(ngm, 16), nd), dim3(256), 0, s, nd, dm, P.c_ptr.p, P.c_row.p, P.c_src.p, ig);
  hipLaunchKernelGGL(k_gj_final_scatter, dim3(8, 1, nd), dim3(256), 0, s, nd, dm, P.src.p, P.dst.p, gg);
  hipLaunchKernelGGL(k_gj_final_sym, dim3(256, 1, nd), dim3(256), 0, s, nd, dm, Sd);
  if (bI && w) {
    hipLaunchKernelGGL(k_gj_final_zg, dim3(cdiv(nm, 64), 1, nd), dim3(256), 0, s, nd, G.nsteps - 1, dm);
    hipLaunchKernelGGL(k_gj_final_w, dim3(cdiv(ngm, 256), 1, nd), dim3(256), 0, s, nd, dm, P.c_ptr.p, P.c_row.p, P.c_src.p, ig, w);
  }
  MI_HIP(hipGetLastError());
}

// Keep the level inverses of every following run (mi_schur_setup_keep_levels): storage for all Z_k (Σ n_level² doubles: 6.2 GB
// at config 3 — this is what 288 GB of HBM are for), the row form of the coupling blocks for the back-substitution, and
// new graphs (the run now ends every step with a copy of the level's inverse).
inline void gj_set_keep(mi_setup_s &P, bool on) {
  if (!P.gj) gj_build(P);
  GjState &G = *P.gj;
  if (G.keep == on) return;
  const int nd = P.ndom;
  // refusals first: the plan stays as it was (a plan left with `keep` set and no level storage would copy into nothing)
  if (on && G.nmax > LV_MAX) raise(MI_ERR_BAD_ARG, "level solves: a level of %d nodes exceeds the %d the back-substitution kernel stages", G.nmax, LV_MAX);
  for (int d = 0; on && d < nd; ++d)
    if (P.dom[d].nlev > 0 && P.dom[d].lev_off[P.dom[d].nlev] != P.dom[d].n_i)
      raise(MI_ERR_BAD_ARG, "level solves: subdomain %d has interior nodes that are not connected to its interface", d);
  MI_HIP(hipStreamSynchronize(P.ctx->stream));
  for (auto &g : G.graph) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
  if (G.solve_graph) { (void)hipGraphExecDestroy(G.solve_graph); G.solve_graph = nullptr; }
  G.keep = on; G.have_levels = false;
  if (!on) { G.zstore.release(); G.gstore.release(); G.ustore.release(); G.sv_in.release(); G.sv_out.release(); return; }
  long long ztot = 0;
  std::vector<int> rp, rc, rs;
  for (int d = 0; d < nd; ++d) {
    const SetupDom &D = P.dom[d];
    if (D.nlev == 0) continue;
    for (int k = 0; k < D.nlev; ++k) {
      GjStep &st = G.steps_h[(size_t)(G.nsteps - 1 - k) * nd + d];
      st.zoff = ztot;
      ztot += ((long long)st.n0 * st.n0 + 31) / 32 * 32;
      st.rptr = 0;
      if (k == 0) continue;
      // rows of C_{k-1} = A_{k, k-1}: from its column form (columns = nodes of level k-1)
      st.rptr = (int)rp.size();
      setup::row_form(st.n0, D.lev_off[k] - D.lev_off[k - 1], P.c_ptr_h.data() + D.cptr_off[k - 1], P.c_row_h.data(), P.c_src_h.data(), rp, rc, rs);
    }
  }
  hipStream_t s = P.ctx->stream;
  G.steps.upload(G.steps_h, s);
  G.r_ptr.upload(rp, s); G.r_col.upload(rc, s); G.r_src.upload(rs, s);
  G.zstore.alloc((size_t)ztot + 32);
  G.gstore.alloc((size_t)P.n_bi + 1); G.ustore.alloc((size_t)P.n_bi + 1);
  G.sv_in.alloc((size_t)P.n_bi + 1); G.sv_out.alloc((size_t)P.n_bi + 1);
}
// The two sweeps of a level solve as plain launches on `s`. Forward: g (level order, gstore) from f, read through `perm`
// (position in level order -> index into f). Backward: u (ustore, level order) for the levels of steps `from` .. 0; from ==
// nsteps - 1 starts with u_0 = Z_0 g_0, a smaller `from` expects the u of step from + 1 in ustore (block_jacobi.hpp forms
// its own level 0). `done` (device flag, may be NULL): set = every launch returns at once.
inline void gj_level_forward(mi_setup_s &P, hipStream_t s, const int *perm, const double *f, const int *done) {
  GjState &G = *P.gj;
  const int nd = P.ndom;
  const GjStep *st = G.steps.p;
  const GjDom *dm = G.doms.p;
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  const double *ii = G.in_ii.p;   // the values of the last run
  for (int step = 0; step < G.nsteps; ++step) {
    const int nm = G.n_step[step];
    if (step > 0) hipLaunchKernelGGL(k_lv_zg, dim3(cdiv(nm, 64), 1, nd), dim3(256), 0, s, step, nd, st, dm, G.zstore.p, G.gstore.p, done);
    hipLaunchKernelGGL(k_lv_g, dim3(cdiv(nm, 256), 1, nd), dim3(256), 0, s, step, nd, st, dm, P.c_ptr.p, P.c_row.p, P.c_src.p, ii, perm, f, G.gstore.p, done);
  }
}
inline void gj_level_backward(mi_setup_s &P, hipStream_t s, int from, const int *done) {
  GjState &G = *P.gj;
  const int nd = P.ndom;
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  for (int step = from; step >= 0; --step) {
    const int nm = G.n_step[step];
    hipLaunchKernelGGL(k_lv_back, dim3(cdiv(nm, 64), 1, nd), dim3(256), 0, s, step, step == G.nsteps - 1 ? 1 : 0, nd, G.steps.p, G.zstore.p, G.gstore.p,
                       G.r_ptr.p, G.r_col.p, G.r_src.p, G.in_ii.p, G.ustore.p, done);
  }
}
inline void gj_level_enqueue(mi_setup_s &P, hipStream_t s, const double *f, double *u) {
  GjState &G = *P.gj;
  gj_level_forward(P, s, P.perm.p, f, nullptr);
  gj_level_backward(P, s, G.nsteps - 1, nullptr);
  hipLaunchKernelGGL(k_lv_scatter, dim3(std::min<long long>(4096, std::max<long long>(1, (P.n_bi + 255) / 256))), dim3(256), 0, s, (long long)P.n_bi,
                     P.perm.p, G.ustore.p, u);
  MI_HIP(hipGetLastError());
}
// u = A_II \ f for all subdomains (concatenated interior vectors in the caller's order), device pointers
inline void gj_level_solve(mi_setup_s &P, const double *f, double *u) {
  if (!P.gj || !P.gj->keep || !P.gj->have_levels) raise(MI_ERR_BAD_ARG, "level solves need mi_schur_setup_keep_levels(plan, 1) and a run after it");
  GjState &G = *P.gj;
  hipStream_t s = P.ctx->stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cap);
  if (cap != hipStreamCaptureStatusNone || env_int("MI355_SETUP_NO_GRAPH", 0)) { gj_level_enqueue(P, s, f, u); return; }   // inside somebody's capture: plain launches
  if (!G.solve_graph) G.solve_graph = capture_graph(s, "level solves", [&] { gj_level_enqueue(P, s, G.sv_in.p, G.sv_out.p); });
  MI_HIP(hipMemcpyAsync(G.sv_in.p, f, sizeof(double) * (size_t)P.n_bi, hipMemcpyDeviceToDevice, s));
  MI_HIP(hipGraphLaunch(G.solve_graph, s));
  MI_HIP(hipMemcpyAsync(u, G.sv_out.p, sizeof(double) * (size_t)P.n_bi, hipMemcpyDeviceToDevice, s));
}

inline void gj_run(mi_setup_s &P, const double *ii_val, const double *ig_val, const double *gg_val, const double *bI, double *Sd, double *w) {
  if (!P.gj) gj_build(P);
  GjState &G = *P.gj;
  if (G.keep) G.have_levels = true;
  hipStream_t s = P.ctx->stream;
  const bool rhs = bI != nullptr && w != nullptr;
  auto cp = [&](double *dst, const double *src, long long cnt) {
    if (cnt > 0) MI_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToDevice, s));
  };
  hipGraphExec_t &ex = G.graph[rhs ? 1 : 0];
  bool plain = G.graph_failed || env_int("MI355_SETUP_NO_GRAPH", 0);
  if (!plain && !ex) {
    try {
      ex = capture_graph(s, "device set-up", [&] {
        gj_enqueue(P, s, G.in_ii.p, G.in_ig.p, G.in_gg.p, rhs ? G.in_bi.p : nullptr, G.out_S.p, rhs ? G.out_w.p : nullptr);
      });
    } catch (const Error &) {                    // a failed capture: plain launches in this run and in every later one
      (void)hipGetLastError();
      G.graph_failed = plain = true;
    }
  }
  if (plain) {
    if (G.keep) cp(G.in_ii.p, ii_val, P.n_ii);   // the level solves read the coupling values from the plan's copy
    gj_enqueue(P, s, ii_val, ig_val, gg_val, rhs ? bI : nullptr, Sd, w);
    return;
  }
  cp(G.in_ii.p, ii_val, P.n_ii); cp(G.in_ig.p, ig_val, P.n_ig); cp(G.in_gg.p, gg_val, P.n_gg);
  if (rhs) cp(G.in_bi.p, bI, P.n_bi);
  MI_HIP(hipGraphLaunch(ex, s));
  cp(Sd, G.out_S.p, P.n_s);
  if (rhs) cp(w, G.out_w.p, P.n_w);
}

// ---------------------------------------------------------------- pinv of well-conditioned blocks = their inverse
// `pinv(S_d, rtol)` keeps the singular values above rtol * σ_max. If 1 / ||S^{-1}||_inf > rtol * ||S||_inf then
// σ_min >= 1 / ||S^{-1}||_2 >= 1 / ||S^{-1}||_inf > rtol ||S||_inf >= rtol σ_max: nothing is dropped and the pseudo-inverse IS the
// inverse — computed by the block Gauss-Jordan kernels above in ~1 ms instead of an eigen-decomposition (~30 ms per block
// through rocSOLVER).
// FLOATING subdomains (no Dirichlet node: pure Neumann problem, `S_d 1 = 0` — at the reference's own partitions, 80-500
// subdomains, almost every block) fail that test by construction. For a symmetric positive semi-definite S whose kernel is
// span{u}, u = 1/sqrt(n):   S^+ = (S + α u u')^{-1} - (1/α) u u'   for any α > 0 (S + α u u' has the eigenpairs of S with
// the zero eigenvalue replaced by α). With α = ||S||_inf the shifted matrix is as well conditioned as S on its range, the
// SAME kernels invert it, and the same certificate on it shows that no OTHER singular value lies below the cut-off. Taken
// when ||S 1||_inf <= rtol max(max_i |S_ii|, ||S||_inf / sqrt(n)): both terms are lower bounds on σ_max and
// λ_min <= u'S u <= ||S 1||_inf, so pinv drops an eigenvalue too (a test against rtol ||S||_inf alone, up to sqrt(n) σ_max,
// would drop eigenvalues in (rtol σ_max, rtol ||S||_inf] that pinv keeps). The result is then accepted only if also
// ||S 1||_inf ||(S + α u u')^{-1}||_inf <= rtol, which bounds the angle between u and the dropped eigenvector. Blocks that
// fail any of these (rank deficiency > 1, a kernel that is not the constants, an eigenvalue near the cut-off) go to the
// spectral route (rocSOLVER dsyevd).
template <bool SIGNED>
__global__ __launch_bounds__(256) void k_rowsum_max_t(int n, const double *__restrict__ A, double *__restrict__ out) {
  __shared__ double sm[NT / 64 + 1];
  double m = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s2 = 0.0;
    for (int c = 0; c < n; ++c) s2 += SIGNED ? A[r + (size_t)c * n] : fabs(A[r + (size_t)c * n]);   // symmetric: column sums = row sums, coalesced this way
    s2 = fabs(s2);
    m = fmax(m, isfinite(s2) ? s2 : INFINITY);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
// max_i |A_ii| (<= ||A||_2), one partial maximum per workgroup as k_rowsum_max_t
__global__ __launch_bounds__(256) void k_diag_max(int n, const double *__restrict__ A, double *__restrict__ out) {
  __shared__ double sm[NT / 64 + 1];
  double m = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    const double a = fabs(A[r + (size_t)r * n]);
    m = fmax(m, isfinite(a) ? a : INFINITY);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
// Probe of the computed inverse: v_j = ±1 (fixed signs), t = (A + c) v with c added to every entry as T = A + c was formed
// before the inversion, then out[blockIdx.x] = max_i |v_i - (Z t)_i| over this workgroup's rows (k_probe_residual).
__device__ __forceinline__ double probe_sign(int j) { return ((unsigned)j * 2654435761u) & 0x10000u ? 1.0 : -1.0; }
__global__ __launch_bounds__(256) void k_probe_apply(int n, const double *__restrict__ A, double c, double *__restrict__ t) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s2 = 0.0;
    for (int j = 0; j < n; ++j) s2 += (A[r + (size_t)j * n] + c) * probe_sign(j);
    t[r] = s2;
  }
}
__global__ __launch_bounds__(256) void k_probe_residual(int n, const double *__restrict__ Z, const double *__restrict__ t,
                                                        double *__restrict__ out) {
  __shared__ double sm[NT / 64 + 1];
  double m = 0.0;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
    double s2 = 0.0;
    for (int j = 0; j < n; ++j) s2 += Z[r + (size_t)j * n] * t[j];
    const double e = fabs(probe_sign(r) - s2);
    m = fmax(m, isfinite(e) ? e : INFINITY);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
}
__global__ __launch_bounds__(256) void k_add_const(long long n, double *__restrict__ A, double c) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) A[e] += c;
}
// dst = src + c (element-wise)
__global__ __launch_bounds__(256) void k_copy_add_const(long long n, const double *__restrict__ src, double *__restrict__ dst, double c) {
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) dst[e] = src[e] + c;
}
inline void pinv_blocks(mi_ctx_s *c, int ndom, const int64_t *n_gamma_d, const double *Sd, double rtol, double *Pi);   // the spectral route: pinv_spectral.hpp
inline std::atomic<long long> &spectral_pinv_calls() { static std::atomic<long long> n{0}; return n; }   // blocks sent to the eigen-decomposition (mi_ctx_query)

// `spd_only` (block_jacobi.hpp: the Schur complements of an SPD matrix are SPD): the plain inverse with its certificate or
// MI_ERR_SINGULAR; the floating and the spectral route are never taken. `failed` (amg_bank_setup.hpp; with spd_only): a block
// that is not finite or misses its certificate does not raise; (*failed)[d] gets the words of the raise, the block's part
// of Pi is left as it was, and the other blocks are finished. Without it the first bad block raises, as before.
inline void pinv_blocks_fast(mi_ctx_s *c, int ndom, const int64_t *n_gamma_d, const double *Sd, double rtol, double *Pi, bool spd_only = false,
                             std::vector<std::string> *failed = nullptr) {
  hipStream_t s = c->stream;
  if (failed) failed->assign((size_t)ndom, std::string());
  auto bad_block = [&](int d, const char *fmt, auto... a) {   // raise, or note the words and go on
    if (!failed) raise(MI_ERR_SINGULAR, fmt, a...);
    char buf[512];
    std::snprintf(buf, sizeof buf, fmt, a...);
    (*failed)[(size_t)d] = buf;
  };
  if (!spd_only && env_int("MI355_PINV_EIG", 0)) { spectral_pinv_calls() += ndom; pinv_blocks(c, ndom, n_gamma_d, Sd, rtol, Pi); return; }
  std::vector<GjStep> st(ndom);
  std::vector<GjDom> dm(ndom);
  size_t tot = 0;
  std::vector<size_t> oT(ndom), o0(ndom), o1(ndom), oP(ndom), off(ndom), ov(ndom);
  size_t run = 0, nsum = 0;
  for (int d = 0; d < ndom; ++d) {
    const size_t n = (size_t)n_gamma_d[d], nn = std::max<size_t>(1, n * n);
    off[d] = run; run += n * n; ov[d] = nsum; nsum += n;
    auto take = [&](size_t cnt) { const size_t o = tot; tot += (cnt + 31) / 32 * 32; return o; };
    oT[d] = take(nn); o0[d] = take(nn); o1[d] = take(nn); oP[d] = take(2 * GJ_B * GJ_B);
  }
  DevBuf<double> pool(tot + 32), norms((size_t)5 * ndom * 8), probe(nsum + 32);
  for (int d = 0; d < ndom; ++d) {
    const int n = (int)n_gamma_d[d];
    st[d] = GjStep{}; st[d].n0 = n; st[d].nb = (n + GJ_B - 1) / GJ_B;
    dm[d] = GjDom{}; dm[d].T = pool.p + oT[d]; dm[d].Z[0] = pool.p + o0[d]; dm[d].Z[1] = pool.p + o1[d]; dm[d].P = pool.p + oP[d];
  }
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  DevBuf<GjStep> std_; DevBuf<GjDom> dmd;
  // One batch: T_d = S_d + shift_d (every entry) for the blocks `ds`, inverted together; norms of S_d (abs row sums), of the
  // inverse, of S_d 1 (signed row sums), the largest |diagonal entry| of S_d, and the probe residual ||v - Z (S_d + shift_d) v||_inf
  // (v = ±1) come back to the host.
  auto batch = [&](const std::vector<int> &ds, const std::vector<double> &shift, std::vector<double> &nS, std::vector<double> &nZ,
                   std::vector<double> &nS1, std::vector<double> &nD, std::vector<double> &nR) {
    std::vector<GjStep> sb; std::vector<GjDom> db;
    int nmax = 1, nbmax = 0;
    for (size_t k = 0; k < ds.size(); ++k) {
      const int d = ds[k], n = (int)n_gamma_d[d];
      sb.push_back(st[d]); db.push_back(dm[d]);
      nmax = std::max(nmax, n); nbmax = std::max(nbmax, st[d].nb);
      if (n) hipLaunchKernelGGL(k_copy_add_const, dim3(std::min(4096, cdiv(n * n, 256))), dim3(256), 0, s, (long long)n * n, Sd + off[d], dm[d].T, shift[k]);
    }
    std_.upload(sb, s); dmd.upload(db, s);
    const int nb_ = (int)ds.size();
    if (nb_ > GJ_MAX_DOM) raise(MI_ERR_BAD_ARG, "pinv: more than %d blocks in one batch", GJ_MAX_DOM);
    gj_block_steps(s, 0, nbmax, nmax, nb_, std_.p, dmd.p);
    for (size_t k = 0; k < ds.size(); ++k) {
      const int d = ds[k], n = (int)n_gamma_d[d];
      if (!n) continue;
      hipLaunchKernelGGL(k_probe_apply, dim3(8), dim3(256), 0, s, n, Sd + off[d], shift[k], probe.p + ov[d]);
      hipLaunchKernelGGL(k_probe_residual, dim3(8), dim3(256), 0, s, n, (const double *)dm[d].Z[st[d].nb & 1], (const double *)probe.p + ov[d],
                         norms.p + (size_t)40 * d + 32);
      hipLaunchKernelGGL(k_rowsum_max_t<false>, dim3(8), dim3(256), 0, s, n, Sd + off[d], norms.p + (size_t)40 * d);
      hipLaunchKernelGGL(k_rowsum_max_t<false>, dim3(8), dim3(256), 0, s, n, dm[d].Z[st[d].nb & 1], norms.p + (size_t)40 * d + 8);
      hipLaunchKernelGGL(k_rowsum_max_t<true>, dim3(8), dim3(256), 0, s, n, Sd + off[d], norms.p + (size_t)40 * d + 16);
      hipLaunchKernelGGL(k_diag_max, dim3(8), dim3(256), 0, s, n, Sd + off[d], norms.p + (size_t)40 * d + 24);
    }
    MI_HIP(hipGetLastError());
    std::vector<double> nh((size_t)40 * ndom);
    MI_HIP(hipMemcpyAsync(nh.data(), norms.p, sizeof(double) * nh.size(), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    nS.assign(ndom, 0.0); nZ.assign(ndom, 0.0); nS1.assign(ndom, 0.0); nD.assign(ndom, 0.0); nR.assign(ndom, 0.0);
    for (int d : ds)
      for (int k = 0; k < 8; ++k) {
        nS[d] = std::max(nS[d], nh[(size_t)40 * d + k]); nZ[d] = std::max(nZ[d], nh[(size_t)40 * d + 8 + k]);
        nS1[d] = std::max(nS1[d], nh[(size_t)40 * d + 16 + k]); nD[d] = std::max(nD[d], nh[(size_t)40 * d + 24 + k]);
        nR[d] = std::max(nR[d], nh[(size_t)40 * d + 32 + k]);
      }
  };
  std::vector<int> all;
  for (int d = 0; d < ndom; ++d) all.push_back(d);
  std::vector<double> nS, nZ, nS1, nD, nR, zero(ndom, 0.0);
  batch(all, zero, nS, nZ, nS1, nD, nR);
  // The certificates below test the computed inverse Z, so they say nothing about its accuracy: without pivoting the block
  // Gauss-Jordan kernels can lose accuracy faster than κ eps: the Schur complement of a short trailing pivot block is formed
  // from the explicit inverse of the block before it (measured: 1e-4 at κ = 1e8, n = 65; 41 % while the pivot inverses
  // were mirrored to symmetry, see gj_invert_block64). A good
  // inverse has |I - Z T| <= c n eps |Z| |T| entry-wise, so ||v - Z T v||_inf <= c n eps ||Z||_inf ||T||_inf for v = ±1;
  // a result whose probe residual exceeds that (c = PROBE_C) is not used, and the block goes to the next route.
  constexpr double PROBE_C = 4.0;
  const double eps = std::numeric_limits<double>::epsilon();
  auto probe_ok = [&](int n, double nT, double nZ_, double res) { return std::isfinite(res) && res <= PROBE_C * n * eps * nT * nZ_; };
  std::vector<int> floating, slow;
  std::vector<double> shift;
  for (int d = 0; d < ndom; ++d) {
    const int n = (int)n_gamma_d[d];
    if (!n) continue;
    if (!std::isfinite(nS[d])) {
      bad_block(d, "mi_nn_pinv: block %d is not finite (mi_schur_setup_run met a singular or indefinite interior block)", d);
      continue;
    }
    const bool inv_ok = std::isfinite(nS[d]) && std::isfinite(nZ[d]) && nZ[d] > 0.0 && 1.0 / nZ[d] > rtol * nS[d] &&
                        probe_ok(n, nS[d], nZ[d], nR[d]);
    if (inv_ok) MI_HIP(hipMemcpyAsync(Pi + off[d], dm[d].Z[st[d].nb & 1], sizeof(double) * (size_t)n * n, hipMemcpyDeviceToDevice, s));
    else if (spd_only) {
      if (!failed) MI_HIP(hipStreamSynchronize(s));   // the copies out of Z above
      bad_block(d, "block %d (%d x %d) is singular or its inverse fails the certificate (probe residual %.3e, bar %.3e)", d, n, n, nR[d],
                PROBE_C * n * eps * nS[d] * nZ[d]);
    }
    // (max |S_ii| and ||S||_inf / sqrt(n) are both <= σ_max: an S 1 this small means pinv drops at least one eigenvalue)
    else if (std::isfinite(nS[d]) && nS[d] > 0.0 && nS1[d] <= rtol * std::max(nD[d], nS[d] / std::sqrt((double)n)) &&
             !env_int("MI355_PINV_NO_SHIFT", 0)) {
      floating.push_back(d);
      shift.push_back(nS[d] / n);                  // α u u' with α = ||S||_inf, u = 1/sqrt(n): every entry + α / n
    } else slow.push_back(d);
  }
  if (!floating.empty()) {
    MI_HIP(hipStreamSynchronize(s));               // the copies out of Z above
    std::vector<double> nS2, nZ2, nS12, nD2, nR2;
    batch(floating, shift, nS2, nZ2, nS12, nD2, nR2);
    for (size_t k = 0; k < floating.size(); ++k) {
      const int d = floating[k], n = (int)n_gamma_d[d];
      const double alpha = shift[k] * n;
      // every eigenvalue of S + α u u' above the cut-off, and u close enough to the eigenvector that is dropped
      const bool ok = std::isfinite(nZ2[d]) && nZ2[d] > 0.0 && 1.0 / nZ2[d] > rtol * nS[d] && nS1[d] * nZ2[d] <= rtol &&
                      probe_ok(n, 2.0 * nS[d], nZ2[d], nR2[d]);   // (||S + α u u'||_inf <= ||S||_inf + α = 2 ||S||_inf)
      if (ok) hipLaunchKernelGGL(k_copy_add_const, dim3(std::min(4096, cdiv(n * n, 256))), dim3(256), 0, s, (long long)n * n,
                                 (const double *)dm[d].Z[st[d].nb & 1], Pi + off[d], -1.0 / (alpha * n));   // - (1/α) u u'
      else slow.push_back(d);
    }
    MI_HIP(hipGetLastError());
  }
  for (int d : slow) { ++spectral_pinv_calls(); pinv_blocks(c, 1, n_gamma_d + d, Sd + off[d], rtol, Pi + off[d]); }
  MI_HIP(hipStreamSynchronize(s));   // the work buffers go out of scope
}

}  // namespace mi
