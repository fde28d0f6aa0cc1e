// Host driver of csrc/amg_plan.hpp (the symbolic phase of the device AMG set-up on frozen aggregates).
// Usage: amg_plan_check FILE...   FILE: whitespace-separated integers
//   n nlevels base rank n_ranks agg_given, then arrays, each as its length followed by its entries:
//   n_l, rowptr, colidx, agg[0] .. agg[agg_given - 1]  (the aggregate pointers beyond agg_given are NULL)
// For every file it prints one JSON line: {"status", "err", "nlev", "bytes", "levels": [{every array of the level}, ...]},
// no levels after a refusal. The weights tw are printed with 17 significant digits. The checks themselves are
// tests/test_amg_refresh_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/amg_plan.hpp"

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

static void print_array(const char *name, const std::vector<int> &v, bool first = false) {
  std::printf("%s\"%s\": [", first ? "" : ", ", name);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%d", k ? ", " : "", v[k]);
  std::printf("]");
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    long long n, nlevels, base, rank, n_ranks, agg_given;
    if (std::fscanf(fp, "%lld %lld %lld %lld %lld %lld", &n, &nlevels, &base, &rank, &n_ranks, &agg_given) != 6 || agg_given < 0) return 2;
    vec n_l, rowptr, colidx;
    std::vector<vec> agg((size_t)agg_given);
    bool ok = read_array(fp, n_l) && read_array(fp, rowptr) && read_array(fp, colidx);
    for (auto &a : agg) ok = ok && read_array(fp, a);
    std::fclose(fp);
    // make_plan trusts the lengths it is told (as the C ABI does): the driver keeps them honest
    if (!ok || (long long)rowptr.size() != n + 1 || n < 1 || (long long)n_l.size() < nlevels || (rowptr.back() - base > (long long)colidx.size())) {
      std::fprintf(stderr, "%s: malformed case\n", argv[f]);
      return 2;
    }
    for (long long l = 0; l < agg_given && l < nlevels; ++l)   // a short array is padded with an id that is out of range
      if ((long long)agg[(size_t)l].size() < n_l[(size_t)l] && n_l[(size_t)l] <= (1ll << 24)) agg[(size_t)l].resize((size_t)n_l[(size_t)l], base - 1);
    std::vector<const int64_t *> ap;
    for (long long l = 0; l + 1 < nlevels || l < agg_given; ++l) ap.push_back(l < agg_given ? agg[(size_t)l].data() : nullptr);
    ap.push_back(nullptr);
    mi::amgp::Plan pl;
    std::string err;
    const int st = mi::amgp::make_plan(n, rowptr.data(), colidx.data(), nlevels, n_l.data(), ap.data(), (int)base, (int)rank, (int)n_ranks, pl, err);
    std::string quoted;
    for (char ch : err) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
    std::printf("{\"status\": %d, \"err\": \"%s\", \"nlev\": %d, \"bytes\": %lld, \"levels\": [", st, quoted.c_str(), pl.nlev, (long long)pl.bytes());
    for (size_t l = 0; l < pl.lv.size(); ++l) {
      const mi::amgp::Level &L = pl.lv[l];
      std::printf("%s{\"n\": %d, \"nc\": %d, ", l ? ", " : "", L.n, L.nc);
      print_array("a_ptr", L.a_ptr, true); print_array("a_col", L.a_col); print_array("diag", L.diag); print_array("sym", L.sym);
      print_array("agg", L.agg); print_array("p_ptr", L.p_ptr); print_array("p_col", L.p_col); print_array("seg_ptr", L.seg_ptr);
      print_array("seg_src", L.seg_src); print_array("r_ptr", L.r_ptr); print_array("r_col", L.r_col); print_array("r_from", L.r_from);
      print_array("ap_ptr", L.ap_ptr); print_array("ap_col", L.ap_col);
      std::printf(", \"tw\": [");
      for (size_t k = 0; k < L.tw.size(); ++k) std::printf("%s%.17g", k ? ", " : "", L.tw[k]);
      std::printf("]}");
    }
    std::printf("]}\n");
  }
  return 0;
}
