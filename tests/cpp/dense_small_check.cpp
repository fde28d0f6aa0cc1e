// CPU check of csrc/dense_small.hpp (host-side Jacobi eigen / SVD used by the eigCG restarts).
// Reads nothing; prints max errors for random cases; exit code 0 when all are below tolerance.
// With the argument `nonfinite`: sym_eig_upper, svd_left and ritz_restart on inputs that hold NaN, +Inf or -Inf in one
// diagonal entry, in one off-diagonal entry or everywhere; one JSON line per case. Every call has to return (the sweeps
// are bounded at 100 and 60) with nev <= m and m * nev entries in G; the values themselves are not checked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../julia-phd-krylov-spdes_amd/csrc/dense_small.hpp"

using namespace mi::dense;

static int nonfinite() {
  const double inf = std::numeric_limits<double>::infinity();
  const double values[3] = {std::numeric_limits<double>::quiet_NaN(), inf, -inf};
  const char *vname[3] = {"nan", "+inf", "-inf"};
  const char *where[3] = {"diagonal", "off-diagonal", "everywhere"};
  int bad = 0;
  for (auto mn : {std::pair<int, int>{3, 1}, {6, 2}, {24, 10}, {70, 33}}) {
    const int m = mn.first, nvec = mn.second, k = 2 * nvec;
    for (int v = 0; v < 3; ++v)
      for (int w = 0; w < 3; ++w) {
        std::mt19937_64 rng(100 * m + 10 * v + w);
        std::normal_distribution<double> nd;
        Mat T((size_t)m * m, 0.0);   // Lanczos-like: upper triangle of a tridiagonal
        for (int i = 0; i < m; ++i) { T[i + (size_t)i * m] = 2.0 + 0.1 * i; if (i) T[(i - 1) + (size_t)i * m] = -1.0; }
        Mat Y((size_t)m * k);
        for (auto &y : Y) y = nd(rng);
        const int i0 = m / 2;
        if (w == 0) { T[i0 + (size_t)i0 * m] = values[v]; Y[(i0 % k) * (size_t)m + i0] = values[v]; }
        if (w == 1) { T[(i0 - 1 >= 0 ? i0 - 1 : 0) + (size_t)(i0 ? i0 : 1) * m] = values[v]; Y[(size_t)((i0 + 1) % k) * m + i0] = values[v]; }
        if (w == 2) {
          for (int j = 0; j < m; ++j)
            for (int i = 0; i <= j; ++i) T[i + (size_t)j * m] = values[v];
          for (auto &y : Y) y = values[v];
        }
        int returned = 0;
        std::vector<double> vals, s;
        Mat V, U;
        sym_eig_upper(m, T.data(), m, vals, V);
        returned += (int)vals.size() == m && V.size() == (size_t)m * m;
        svd_left(m, k, Y, s, U);
        returned += (int)s.size() == k && U.size() == (size_t)m * k;
        Ritz R = ritz_restart(T.data(), m, m, nvec);
        returned += (int)R.vals.size() == R.nev;
        const bool ok = returned == 3 && R.nev >= 0 && R.nev <= m && R.G.size() == (size_t)m * R.nev;
        bad += !ok;
        std::printf("{\"m\": %d, \"nvec\": %d, \"value\": \"%s\", \"where\": \"%s\", \"returned\": %d, \"nev\": %d, \"g_size\": %zu}\n",
                    m, nvec, vname[v], where[w], returned, R.nev, R.G.size());
      }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "nonfinite")) return nonfinite();
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nd;
  double worst = 0.0;
  for (int n : {1, 2, 3, 7, 24, 61}) {
    Mat A((size_t)n * n);
    for (int j = 0; j < n; ++j)
      for (int i = 0; i <= j; ++i) A[i + (size_t)j * n] = A[j + (size_t)i * n] = nd(rng);
    std::vector<double> w;
    Mat V;
    sym_eig_upper(n, A.data(), n, w, V);
    double err = 0.0, orth = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j && w[j] < w[j - 1]) err = 1.0;
      for (int i = 0; i < n; ++i) {
        double av = 0.0, vv = 0.0;
        for (int l = 0; l < n; ++l) { av += A[i + (size_t)l * n] * V[l + (size_t)j * n]; vv += V[l + (size_t)i * n] * V[l + (size_t)j * n]; }
        err = std::max(err, std::fabs(av - w[j] * V[i + (size_t)j * n]));
        orth = std::max(orth, std::fabs(vv - (i == j)));
      }
    }
    std::printf("eig n=%d resid=%.2e orth=%.2e\n", n, err, orth);
    worst = std::max(worst, std::max(err, orth) / std::max(1.0, (double)n));
  }
  for (auto mk : {std::pair<int, int>{24, 20}, {9, 12}, {30, 6}}) {
    const int m = mk.first, k = mk.second;
    Mat Y((size_t)m * k);
    for (auto &y : Y) y = nd(rng);
    for (int i = 0; i < m; ++i) Y[i + (size_t)(k - 1) * m] = Y[i] * 2.0;  // rank deficiency 1
    std::vector<double> s;
    Mat U;
    svd_left(m, k, Y, s, U);
    // check: U_r' Y has row norms s, and U_r orthonormal; projector U_r U_r' Y = Y
    int r = 0;
    for (int j = 0; j < std::min(m, k); ++j) r += s[j] > 1e-12 * s[0];
    double orth = 0.0, rec = 0.0;
    for (int a = 0; a < r; ++a)
      for (int b = 0; b < r; ++b) {
        double d = 0.0;
        for (int i = 0; i < m; ++i) d += U[i + (size_t)a * m] * U[i + (size_t)b * m];
        orth = std::max(orth, std::fabs(d - (a == b)));
      }
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < m; ++i) {
        double p = 0.0;
        for (int a = 0; a < r; ++a) {
          double c = 0.0;
          for (int l = 0; l < m; ++l) c += U[l + (size_t)a * m] * Y[l + (size_t)j * m];
          p += U[i + (size_t)a * m] * c;
        }
        rec = std::max(rec, std::fabs(p - Y[i + (size_t)j * m]));
      }
    std::printf("svd %dx%d rank=%d (expect %d) orth=%.2e rec=%.2e\n", m, k, r, std::min(m, k - 1), orth, rec);
    if (r != std::min(m, k - 1)) worst = 1.0;
    worst = std::max(worst, std::max(orth, rec));
  }
  // Ritz restart on a Lanczos-like tridiagonal: G has orthonormal columns, vals are Ritz values of Tm on span(G)
  {
    const int m = 24, nvec = 10;
    Mat T((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) { T[i + (size_t)i * m] = 2.0 + 0.1 * i; if (i) T[(i - 1) + (size_t)i * m] = -1.0; }
    Ritz R = ritz_restart(T.data(), m, m, nvec);
    double orth = 0.0;
    for (int a = 0; a < R.nev; ++a)
      for (int b = 0; b < R.nev; ++b) {
        double d = 0.0;
        for (int i = 0; i < m; ++i) d += R.G[i + (size_t)a * m] * R.G[i + (size_t)b * m];
        orth = std::max(orth, std::fabs(d - (a == b)));
      }
    std::printf("ritz nev=%d orth=%.2e vals[0]=%.12f\n", R.nev, orth, R.vals[0]);
    if (R.nev < nvec || R.nev > 2 * nvec) worst = 1.0;
    worst = std::max(worst, orth);
  }
  std::printf("worst=%.2e\n", worst);
  return worst < 1e-12 ? 0 : 1;
}
