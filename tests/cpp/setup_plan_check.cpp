// Host driver of csrc/setup_plan.hpp (the symbolic half of the level set-up) and of bj::make_split (block_jacobi.hpp) on top of it.
// Usage: setup_plan_check FILE...   FILE: whitespace-separated integers, arrays as their length followed by their entries
//   plan mode   0 ndom base, then n_gamma_d, n_i, and per subdomain ii_colptr, ii_rowval, ig_colptr, ig_rowval, gg_colptr,
//               gg_rowval (an empty array is passed as NULL)
//   split mode  1 n nb base has_seeds, then colptr, rowval of the full pattern [, seed_ptr, seed_idx]
// For every file it prints one JSON line. Plan mode: {"status", "err", the totals, the plan-wide arrays, "dom": the
// records, each with the row forms (setup::row_form) of its coupling blocks C_0 .. C_{nlev-2} and of B appended to one
// r_ptr / r_col / r_src, block q starting at r_ptr[r_off[q]]}. Split mode: {"status", "err", "G", "I", "ncomp" and, from the
// plan of the split, "lev_off" and "n_i" per block}. After a refusal only status and err are meaningful. The checks
// themselves are tests/test_setup_plan_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/block_jacobi.hpp"
#include "../../julia-phd-krylov-spdes_amd/csrc/setup_plan.hpp"

using vec = std::vector<int64_t>;

static bool read_array(FILE *fp, vec &v) {
  long long len = 0;
  if (std::fscanf(fp, "%lld", &len) != 1 || len < 0) return false;
  v.resize((size_t)len);
  for (auto &x : v) {
    long long t;
    if (std::fscanf(fp, "%lld", &t) != 1) return false;
    x = t;
  }
  return true;
}

template <typename T>
static void print_array(const char *name, const std::vector<T> &v, const char *lead = ", ") {
  std::printf("%s\"%s\": [", lead, name);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v[k]);
  std::printf("]");
}
template <typename T>
static void print_lists(const char *name, const std::vector<std::vector<T>> &v) {
  std::printf(", \"%s\": [", name);
  for (size_t d = 0; d < v.size(); ++d) {
    std::printf("%s[", d ? ", " : "");
    for (size_t k = 0; k < v[d].size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v[d][k]);
    std::printf("]");
  }
  std::printf("]");
}
static void print_status(int st, const std::string &err) {
  std::string quoted;
  for (char ch : err) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
  std::printf("{\"status\": %d, \"err\": \"%s\"", st, quoted.c_str());
}

static int plan_mode(FILE *fp, const char *name) {
  long long ndom, base;
  if (std::fscanf(fp, "%lld %lld", &ndom, &base) != 2 || ndom < 0) return 2;
  vec n_g, n_i;
  std::vector<vec> arr[6];
  bool ok = read_array(fp, n_g) && read_array(fp, n_i);
  for (auto &a : arr) a.resize((size_t)ndom);
  for (long long d = 0; d < ndom && ok; ++d)
    for (auto &a : arr) ok = ok && read_array(fp, a[d]);
  if (!ok || (long long)n_g.size() != ndom || (long long)n_i.size() != ndom) { std::fprintf(stderr, "%s: malformed case\n", name); return 2; }
  std::vector<const int64_t *> ptr[6];
  for (int q = 0; q < 6; ++q)
    for (long long d = 0; d < ndom; ++d) ptr[q].push_back(arr[q][d].empty() ? nullptr : arr[q][d].data());
  mi::setup::Input in;
  in.ndom = ndom; in.base = (int)base; in.n_gamma_d = n_g.data(); in.n_i = n_i.data();
  in.ii_ptr = ptr[0].data(); in.ii_idx = ptr[1].data(); in.ig_ptr = ptr[2].data(); in.ig_idx = ptr[3].data();
  in.gg_ptr = ptr[4].data(); in.gg_idx = ptr[5].data();
  mi::setup::Plan P;
  std::string err;
  const int st = mi::setup::make_plan(in, P, err);
  print_status(st, err);
  if (st != mi::setup::OK) { std::printf("}\n"); return 0; }
  std::printf(", \"ndom\": %d, \"n_ii\": %lld, \"n_ig\": %lld, \"n_gg\": %lld, \"n_bi\": %lld, \"n_s\": %lld, \"n_w\": %lld", P.ndom, P.n_ii, P.n_ig,
              P.n_gg, P.n_bi, P.n_s, P.n_w);
  print_array("src", P.src_h); print_array("dst", P.dst_h); print_array("perm", P.perm_h);
  print_array("c_ptr", P.c_ptr_h); print_array("c_row", P.c_row_h); print_array("c_src", P.c_src_h);
  std::printf(", \"dom\": [");
  for (int d = 0; d < P.ndom; ++d) {
    const mi::setup::Dom &D = P.dom[d];
    std::printf("%s{\"n_g\": %d, \"n_i\": %d, \"nlev\": %d, \"max_lev\": %d, \"g_e0\": %lld, \"g_e1\": %lld, \"ii_val_off\": %lld, \"ig_val_off\": %lld, "
                "\"gg_val_off\": %lld, \"bi_off\": %lld, \"s_off\": %lld, \"w_off\": %lld, \"bptr_off\": %d",
                d ? ", " : "", D.n_g, D.n_i, D.nlev, D.max_lev, D.g_e0, D.g_e1, D.ii_val_off, D.ig_val_off, D.gg_val_off, D.bi_off, D.s_off, D.w_off,
                D.bptr_off);
    print_array("lev_off", D.lev_off); print_array("d_e0", D.d_e0); print_array("cptr_off", D.cptr_off);
    std::vector<int> r_off, r_ptr, r_col, r_src;
    for (int k = 0; k + 1 < D.nlev; ++k) {          // C_k = A_{k+1,k}: rows level k + 1, columns level k
      r_off.push_back((int)r_ptr.size());
      mi::setup::row_form(D.lev_off[k + 2] - D.lev_off[k + 1], D.lev_off[k + 1] - D.lev_off[k], P.c_ptr_h.data() + D.cptr_off[k], P.c_row_h.data(),
                          P.c_src_h.data(), r_ptr, r_col, r_src);
    }
    r_off.push_back((int)r_ptr.size());             // B: rows level 0, columns Γ_d
    mi::setup::row_form(D.nlev ? D.lev_off[1] : 0, D.n_g, P.c_ptr_h.data() + D.bptr_off, P.c_row_h.data(), P.c_src_h.data(), r_ptr, r_col, r_src);
    print_array("r_off", r_off); print_array("r_ptr", r_ptr); print_array("r_col", r_col); print_array("r_src", r_src);
    std::printf("}");
  }
  std::printf("]}\n");
  return 0;
}

static int split_mode(FILE *fp, const char *name) {
  long long n, nb, base, has_seeds;
  if (std::fscanf(fp, "%lld %lld %lld %lld", &n, &nb, &base, &has_seeds) != 4 || n < 0) return 2;
  vec cp, ri, sq, sx;
  bool ok = read_array(fp, cp) && read_array(fp, ri);
  if (has_seeds) ok = ok && read_array(fp, sq) && read_array(fp, sx);
  if (!ok || (long long)cp.size() != n + 1) { std::fprintf(stderr, "%s: malformed case\n", name); return 2; }
  for (auto *v : {&cp, &ri, &sq, &sx})
    for (auto &x : *v) x -= base;                   // as BlockJacobiOp hands them over
  mi::bj::Split S;
  std::string err;
  static const int64_t none = 0;
  if (!mi::bj::make_split(n, cp.data(), ri.data(), nb, has_seeds ? sq.data() : nullptr, sx.empty() ? &none : sx.data(), (int)base, S, err)) {
    print_status(1, err);
    std::printf("}\n");
    return 0;
  }
  vec n_g((size_t)nb), n_i((size_t)nb);
  std::vector<const int64_t *> p[6];
  auto at = [](const vec &v) { return v.empty() ? &none : v.data(); };
  for (long long d = 0; d < nb; ++d) {
    n_g[d] = (int64_t)S.G[d].size(); n_i[d] = (int64_t)S.I[d].size();
    p[0].push_back(S.ii_ptr[d].data()); p[1].push_back(at(S.ii_idx[d])); p[2].push_back(S.ig_ptr[d].data()); p[3].push_back(at(S.ig_idx[d]));
    p[4].push_back(S.gg_ptr[d].data()); p[5].push_back(at(S.gg_idx[d]));
  }
  mi::setup::Input in;
  in.ndom = nb; in.base = 0; in.n_gamma_d = n_g.data(); in.n_i = n_i.data();
  in.ii_ptr = p[0].data(); in.ii_idx = p[1].data(); in.ig_ptr = p[2].data(); in.ig_idx = p[3].data(); in.gg_ptr = p[4].data(); in.gg_idx = p[5].data();
  mi::setup::Plan P;
  const int st = mi::setup::make_plan(in, P, err);
  print_status(st, err);
  if (st != mi::setup::OK) { std::printf("}\n"); return 0; }
  print_lists("G", S.G); print_lists("I", S.I); print_array("ncomp", S.ncomp); print_array("n_i", n_i);
  std::vector<std::vector<int>> lev;
  for (auto &D : P.dom) lev.push_back(D.lev_off);
  print_lists("lev_off", lev);
  std::printf("}\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    long long mode = -1;
    int rc = 2;
    if (std::fscanf(fp, "%lld", &mode) == 1) rc = mode == 0 ? plan_mode(fp, argv[f]) : split_mode(fp, argv[f]);
    std::fclose(fp);
    if (rc) return rc;
  }
  return 0;
}
