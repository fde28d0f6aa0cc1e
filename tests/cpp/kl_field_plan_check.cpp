// Host driver of csrc/kl_field_plan.hpp (the tiling and the index plan of the realization sampler).
// Usage: kl_field_plan_check FILE...   FILE: whitespace-separated integers
//   "tiling" n m nreal                          -> {"row_tiles", "real_blocks", "coord_col_blocks", "coord_splits", ...}
//   "plan" n ndom base, then arrays, each as its length followed by its entries: n_d, md, inds
// For every file it prints one JSON line; a plan comes with every array, none after a refusal. The checks themselves are
// tests/test_kl_field_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/kl_field_plan.hpp"

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
    char kind[16] = {0};
    if (std::fscanf(fp, "%15s", kind) != 1) return 2;
    if (!std::strcmp(kind, "tiling")) {
      long long n, m, nreal;
      if (std::fscanf(fp, "%lld %lld %lld", &n, &m, &nreal) != 3) return 2;
      std::fclose(fp);
      const mi::KlfTiling t = mi::klf_tiling(n, m, nreal);
      std::printf("{\"row_tile\": %d, \"mode_chunk\": %d, \"real_block\": %d, \"row_tiles\": %d, \"real_blocks\": %d, \"coord_col_blocks\": %d, "
                  "\"coord_splits\": %d, \"coord_tiles_per_split\": %d, \"rb_in_use\": %d}\n",
                  mi::KLF_ROW_TILE, mi::KLF_MODE_CHUNK, mi::KLF_RB, t.row_tiles, t.real_blocks, t.coord_col_blocks, t.coord_splits,
                  t.coord_tiles_per_split, mi::klf_rb_in_use((int)std::min<long long>(nreal, mi::KLF_RB)));
      continue;
    }
    long long n, ndom, base;
    if (std::fscanf(fp, "%lld %lld %lld", &n, &ndom, &base) != 3) return 2;
    vec n_d, md, inds;
    const bool ok = read_array(fp, n_d) && read_array(fp, md) && read_array(fp, inds);
    std::fclose(fp);
    // make_dd_plan trusts the lengths it is told (as the C ABI does): the driver keeps them honest. A refusal comes before
    // anything of `inds` is read, so short arrays of a refused case are padded, never read past.
    if (!ok || (long long)n_d.size() < ndom || (long long)md.size() < ndom) { std::fprintf(stderr, "%s: malformed case\n", argv[f]); return 2; }
    long long need = 0;
    for (long long d = 0; d < ndom; ++d) need += n_d[(size_t)d] > 0 && n_d[(size_t)d] <= (1ll << 24) ? n_d[(size_t)d] : 0;
    if ((long long)inds.size() < need) inds.resize((size_t)need, base - 1);
    mi::klfp::Plan pl;
    std::string err;
    const int st = mi::klfp::make_dd_plan(n, ndom, n_d.data(), md.data(), inds.data(), (int)base, pl, err);
    std::string quoted;
    for (char ch : err) { if (ch == '"' || ch == '\\') quoted += '\\'; quoted += ch; }
    std::printf("{\"status\": %d, \"err\": \"%s\"", st, quoted.c_str());
    if (st == mi::klfp::OK) {
      std::printf(", \"nloc\": %d, \"nred\": %d, \"cnt_max\": %d, \"md_max\": %d, \"bytes\": %lld", pl.nloc, pl.nred, pl.cnt_max, pl.md_max, (long long)pl.bytes());
      print_array("y_off", pl.y_off); print_array("t_off", pl.t_off); print_array("phid_off", pl.phid_off);
      print_array("own_ptr", pl.own_ptr); print_array("own_pos", pl.own_pos);
      std::vector<int> td, tr;
      for (const mi::klfp::Tile &t : pl.tiles) { td.push_back(t.d); tr.push_back(t.row0); }
      print_array("tile_d", td); print_array("tile_row0", tr);
    }
    std::printf("}\n");
  }
  return 0;
}
