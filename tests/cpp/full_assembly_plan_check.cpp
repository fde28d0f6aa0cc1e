// Host driver of csrc/full_assembly_plan.hpp (the row-owned index plan of the full-system assembly).
// Usage: full_assembly_plan_check FILE...   FILE: whitespace-separated numbers
//   nel n_node base n with_pattern, then arrays, each as its length followed by its entries:
//   cells (3 nel integers), point_marker (n_node integers), rowptr, colidx (integers; read but not passed on when with_pattern
//   is 0), points (2 n_node doubles, written as C99 hexadecimal floats so that no bit is lost)
// For every file it prints one JSON line; a plan comes with every array, none after a refusal. The checks themselves are
// tests/test_full_assembly_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/full_assembly_plan.hpp"

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

static bool read_doubles(FILE *fp, std::vector<double> &v) {
  long long len = 0;
  if (std::fscanf(fp, "%lld", &len) != 1 || len < 0) return false;
  v.resize((size_t)len);
  for (auto &x : v)
    if (std::fscanf(fp, "%la", &x) != 1) return false;
  return true;
}

template <class T>
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
    long long nel, n_node, base, n, with_pattern;
    if (std::fscanf(fp, "%lld %lld %lld %lld %lld", &nel, &n_node, &base, &n, &with_pattern) != 5) return 2;
    vec cells, marker, rowptr, colidx;
    std::vector<double> points;
    const bool ok = read_array(fp, cells) && read_array(fp, marker) && read_array(fp, rowptr) && read_array(fp, colidx) && read_doubles(fp, points);
    std::fclose(fp);
    // make_plan trusts the lengths it is told (as the C ABI does): the driver keeps them honest. The size refusals come
    // before anything is read, so the arrays of such a case may be short.
    const bool sized = nel >= 1 && 4 * nel < (1ll << 31) && n_node >= 1 && n_node < (1ll << 31);
    if (!ok || (sized && ((long long)cells.size() != 3 * nel || (long long)marker.size() != n_node || (long long)points.size() != 2 * n_node)) ||
        (sized && with_pattern && (n < 0 || (long long)rowptr.size() != n + 1 || (long long)colidx.size() != rowptr.back() - base))) {
      // (colidx is compared only after every rowptr entry has matched, so rowptr[n] - base entries are all that is read)
      std::fprintf(stderr, "%s: malformed case\n", argv[f]);
      return 2;
    }
    mi::fap::Plan pl;
    std::string err;
    const int st = mi::fap::make_plan(nel, n_node, cells.data(), (int)base, points.data(), marker.data(), n, with_pattern ? rowptr.data() : nullptr,
                                      with_pattern ? colidx.data() : nullptr, pl, err);
    std::string quoted;
    for (char ch : err) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
    std::printf("{\"status\": %d, \"err\": \"%s\", \"fa_rows\": %d, \"fa_seg\": %d, \"fa_dir\": %u", st, quoted.c_str(), mi::FA_ROWS, mi::FA_SEG, mi::FA_DIR);
    if (st == mi::fap::OK) {
      std::printf(", \"n\": %d, \"bytes\": %lld", pl.n, (long long)pl.bytes());
      print_array("cells", pl.cells); print_array("node_row", pl.node_row); print_array("rowptr", pl.rowptr); print_array("colidx", pl.colidx);
      print_array("diag_pos", pl.diag_pos); print_array("inc_ptr", pl.inc_ptr); print_array("inc_code", pl.inc_code);
      print_array("inc_pos", pl.inc_pos); print_array("blk_row", pl.blk_row);
    }
    std::printf("}\n");
  }
  return 0;
}
