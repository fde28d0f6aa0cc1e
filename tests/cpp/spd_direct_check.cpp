// CPU check of csrc/spd_direct_plan.hpp (the symbolic phase of the sparse direct preconditioner).
// Usage: spd_direct_check P SIGMA_MAX FILE...   FILE: "n nnz" then colptr (n + 1) and rowval (nnz), 0-based, whitespace
// separated. For every file it checks that each node is in exactly one piece or in Σ, that no edge joins two different
// pieces, that pieces have at most P nodes, that Σ_i, the slots and the entry destinations are consistent, and that a
// second run gives the identical plan. Prints one JSON line per file (pieces, |Σ|, orphans, single-node pieces, pieces
// without a Σ neighbour, and the node -> piece map, -1 = Σ);
// exit code 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/spd_direct_plan.hpp"

using namespace mi::spd;

static bool same(const Plan &a, const Plan &b) {
  return a.piece_of == b.piece_of && a.piece_ptr == b.piece_ptr && a.piece_node == b.piece_node && a.sigma == b.sigma &&
         a.sig_ptr == b.sig_ptr && a.sig_idx == b.sig_idx && a.slot_ptr == b.slot_ptr && a.slot == b.slot && a.dst == b.dst &&
         a.orphan == b.orphan;
}

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s P SIGMA_MAX FILE...\n", argv[0]); return 2; }
  const int P = std::atoi(argv[1]), smax = std::atoi(argv[2]);
  int bad = 0;
  for (int f = 3; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    long long n = 0, nnz = 0;
    if (std::fscanf(fp, "%lld %lld", &n, &nnz) != 2) return 2;
    std::vector<int64_t> cp(n + 1), rv(nnz);
    for (auto &v : cp) if (std::fscanf(fp, "%ld", &v) != 1) return 2;
    for (auto &v : rv) if (std::fscanf(fp, "%ld", &v) != 1) return 2;
    std::fclose(fp);
    Plan a, b;
    std::string err;
    const int st = make_plan((int)n, cp.data(), rv.data(), P, smax, a, err);
    const int st2 = make_plan((int)n, cp.data(), rv.data(), P, smax, b, err);
    std::vector<std::string> why;
    if (st != st2 || !same(a, b)) why.push_back("two runs differ");
    if (st == BAD_PATTERN) {   // nothing else to check
      std::printf("{\"file\": \"%s\", \"status\": %d, \"n\": %lld, \"ok\": false, \"why\": \"%s\", \"piece_of\": []}\n", argv[f], st, n, err.c_str());
      ++bad;
      continue;
    }
    // every node in exactly one piece or in Σ
    std::vector<int> seen(n, 0);
    for (int i = 0; i < a.n_pieces(); ++i) {
      const int ni = a.piece_ptr[i + 1] - a.piece_ptr[i];
      if (ni < 1 || ni > P) why.push_back("piece size " + std::to_string(ni));
      for (int p = a.piece_ptr[i]; p < a.piece_ptr[i + 1]; ++p) {
        const int v = a.piece_node[p];
        seen[v]++;
        if (a.piece_of[v] != i || a.local[v] != p - a.piece_ptr[i]) why.push_back("piece map of node " + std::to_string(v));
      }
    }
    for (int s = 0; s < a.n_sigma(); ++s) {
      seen[a.sigma[s]]++;
      if (a.piece_of[a.sigma[s]] != -1 || a.local[a.sigma[s]] != s) why.push_back("Σ map of node " + std::to_string(a.sigma[s]));
    }
    for (int v = 0; v < n; ++v) if (seen[v] != 1) { why.push_back("node " + std::to_string(v) + " seen " + std::to_string(seen[v]) + " times"); break; }
    // no edge between two different pieces
    for (int c = 0; c < n; ++c)
      for (int64_t k = cp[c]; k < cp[c + 1]; ++k) {
        const int r = (int)rv[k];
        if (a.piece_of[r] >= 0 && a.piece_of[c] >= 0 && a.piece_of[r] != a.piece_of[c]) { why.push_back("edge between pieces"); c = (int)n; break; }
      }
    if (st == OK) {
      // Σ_i = exactly the Σ neighbours of piece i; slots list every (piece, Σ node) pair once, ascending
      std::vector<std::set<int>> nb(a.n_pieces());
      for (int c = 0; c < n; ++c)
        for (int64_t k = cp[c]; k < cp[c + 1]; ++k) {
          const int r = (int)rv[k];
          if (a.piece_of[r] >= 0 && a.piece_of[c] < 0) nb[a.piece_of[r]].insert(a.local[c]);
        }
      for (int i = 0; i < a.n_pieces(); ++i)
        if (std::vector<int>(nb[i].begin(), nb[i].end()) != std::vector<int>(a.sig_idx.begin() + a.sig_ptr[i], a.sig_idx.begin() + a.sig_ptr[i + 1]))
          why.push_back("Σ_" + std::to_string(i));
      for (int s = 0; s < a.n_sigma(); ++s) {
        for (int t = a.slot_ptr[s]; t < a.slot_ptr[s + 1]; ++t)
          if (a.sig_idx[a.slot[t]] != s || (t > a.slot_ptr[s] && a.slot[t] <= a.slot[t - 1])) why.push_back("slots of Σ node");
        if ((a.slot_ptr[s] == a.slot_ptr[s + 1]) != std::binary_search(a.orphan.begin(), a.orphan.end(), s)) why.push_back("orphans");
      }
      // every used destination is distinct and inside the work buffer
      std::set<int64_t> d;
      for (int64_t k = 0; k < nnz; ++k)
        if (a.dst[k] >= 0 && (a.dst[k] >= a.work_total() || !d.insert(a.dst[k]).second)) { why.push_back("destinations"); break; }
    }
    if (!why.empty()) ++bad;
    int singles = 0, isolated = 0;   // pieces of one node; pieces without a Σ neighbour
    for (int i = 0; i < a.n_pieces(); ++i) {
      singles += a.piece_ptr[i + 1] - a.piece_ptr[i] == 1;
      if (st == OK) isolated += a.sig_ptr[i + 1] == a.sig_ptr[i];
    }
    std::printf("{\"file\": \"%s\", \"status\": %d, \"n\": %lld, \"pieces\": %d, \"sigma\": %d, \"orphans\": %d, \"singles\": %d, "
                "\"isolated\": %d, \"ok\": %s, \"why\": \"%s\", \"piece_of\": [",
                argv[f], st, n, a.n_pieces(), a.n_sigma(), (int)a.orphan.size(), singles, isolated, why.empty() ? "true" : "false",
                why.empty() ? "" : why[0].c_str());
    for (int v = 0; v < n; ++v) std::printf(v ? ", %d" : "%d", a.piece_of[v]);
    std::printf("]}\n");
  }
  return bad ? 1 : 0;
}
