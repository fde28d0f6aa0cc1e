// Host driver of csrc/full_split_plan.hpp (the interior/Γ split that the LORASC and the induced operator share).
// Usage: full_split_check FILE...   FILE: whitespace-separated integers
//   ndom n n_gamma base gathered, then arrays, each as its length followed by its entries:
//   n_i, plan_n_i, [gathered: n_gamma_d, plan_n_gamma_d,] pos_I[0] .. pos_I[ndom-1], pos_gamma,
//   [gathered: gather[0] .. gather[ndom-1], node_cnt,] and per subdomain colptr, rowval and one flag (1: the value array is NULL).
// For every file it prints one JSON line: {"status", "err", "n_I", "n_g", "nnz", "totg"} and every array of the plan,
// empty after a refusal. The checks themselves are tests/test_full_split_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/full_split_plan.hpp"

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
static void print_array(const char *name, const std::vector<T> &v) {
  std::printf(", \"%s\": [", name);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v[k]);
  std::printf("]");
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    long long ndom, n, n_gamma, base, gathered;
    if (std::fscanf(fp, "%lld %lld %lld %lld %lld", &ndom, &n, &n_gamma, &base, &gathered) != 5 || ndom < 0) return 2;
    vec n_i, plan_n_i, n_gd, plan_n_gd, pos_g, cnt;
    std::vector<vec> pos_I((size_t)ndom), gather((size_t)ndom), colptr((size_t)ndom), rowval((size_t)ndom);
    std::vector<int64_t> val_null((size_t)ndom, 0);
    bool ok = read_array(fp, n_i) && read_array(fp, plan_n_i);
    if (gathered) ok = ok && read_array(fp, n_gd) && read_array(fp, plan_n_gd);
    for (auto &p : pos_I) ok = ok && read_array(fp, p);
    ok = ok && read_array(fp, pos_g);
    if (gathered) {
      for (auto &g : gather) ok = ok && read_array(fp, g);
      ok = ok && read_array(fp, cnt);
    }
    for (long long d = 0; d < ndom && ok; ++d) {
      long long flag = 0;
      ok = read_array(fp, colptr[d]) && read_array(fp, rowval[d]) && std::fscanf(fp, "%lld", &flag) == 1;
      val_null[d] = flag;
    }
    std::fclose(fp);
    if (!ok || (long long)n_i.size() != ndom || (long long)plan_n_i.size() != ndom) { std::fprintf(stderr, "%s: malformed case\n", argv[f]); return 2; }
    std::vector<const int64_t *> pI, gp, cp, rv;
    std::vector<const double *> nz;
    const double some_value = 0.0;           // make_plan looks at the value arrays for NULL only
    for (long long d = 0; d < ndom; ++d) {
      pI.push_back(pos_I[d].empty() ? nullptr : pos_I[d].data());
      gp.push_back(gather[d].empty() ? nullptr : gather[d].data());
      cp.push_back(colptr[d].empty() ? nullptr : colptr[d].data());
      rv.push_back(rowval[d].empty() ? nullptr : rowval[d].data());
      nz.push_back(val_null[d] ? nullptr : &some_value);
    }
    mi::split::Input in;
    in.ndom = ndom; in.n = n; in.n_gamma = n_gamma; in.base = (int)base;
    in.n_i = n_i.data(); in.plan_n_i = plan_n_i.data(); in.pos_I = pI.data(); in.pos_g = pos_g.data();
    in.colptr = cp.data(); in.rowval = rv.data(); in.nzval = nz.data();
    if (gathered) { in.n_gamma_d = n_gd.data(); in.plan_n_gamma_d = plan_n_gd.data(); in.gather = gp.data(); in.node_cnt = cnt.data(); }
    mi::split::Plan pl;
    std::string err;
    const int st = mi::split::make_plan(in, pl, err);
    std::string quoted;
    for (char ch : err) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
    std::printf("{\"status\": %d, \"err\": \"%s\", \"n_I\": %d, \"n_g\": %d, \"nnz\": %lld, \"totg\": %lld", st, quoted.c_str(), pl.n_I, pl.n_g,
                (long long)pl.nnz, (long long)pl.totg);
    if (st != mi::split::OK) pl = mi::split::Plan{};
    print_array("pos_I", pl.pos_I); print_array("pos_g", pl.pos_g); print_array("gseg_ptr", pl.gseg_ptr); print_array("seg_ptr", pl.seg_ptr);
    print_array("c_row", pl.c_row); print_array("c_src", pl.c_src); print_array("r_ptr", pl.r_ptr); print_array("r_loc", pl.r_loc);
    print_array("r_gam", pl.r_gam); print_array("r_src", pl.r_src); print_array("voff", pl.voff); print_array("ioff", pl.ioff);
    print_array("goff", pl.goff);
    std::printf("}\n");
  }
  return 0;
}
