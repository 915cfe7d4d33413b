// Stand-alone check of the plan of the RBF kernel expectations (csrc/psi_plan.hpp) on the CPU: a table of splits and chunks as literal
// numbers, then a grid of shapes and of what the caller asks for, exit 1 with a message on the first violated invariant.  Built and run by
// tests/test_psi_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "psi_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static const char* g_call = "";      // the case at hand: which plan, its shape, and what is asked for as bits (psi2 | g_psi1, g_psi2 << 1, d_Z << 2)
static long long g_n;
static int g_M, g_D, g_asked;
#define REQUIRE(cond, ...)                                                          \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      fprintf(stderr, "psi_plan_check: %s n=%lld M=%d D=%d asked=%d\n  violated: %s\n  ", g_call, g_n, g_M, g_D, g_asked, #cond); \
      fprintf(stderr, __VA_ARGS__);                                                 \
      fprintf(stderr, "\n");                                                        \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

struct Row { int64_t n; int M; int64_t f_rows; int f_ns; int64_t g_rows; int g_ns; int64_t z_rows; int z_nc; };
static const Row TABLE[] = {
    {1, 1, 16, 1, 16, 1, 1, 1},           {17, 1, 32, 1, 32, 1, 17, 1},          {65, 17, 48, 2, 48, 2, 65, 1},
    {129, 33, 48, 3, 48, 3, 129, 1},      {200, 50, 64, 4, 64, 4, 200, 1},       {257, 16, 64, 5, 64, 5, 129, 2},
    {601, 5, 64, 10, 64, 10, 201, 3},     {1000, 128, 64, 16, 64, 16, 250, 4},   {4097, 2048, 4112, 1, 144, 29, 241, 17},
    {40000, 128, 352, 114, 80, 500, 255, 157}, {45000, 256, 1456, 31, 176, 256, 256, 176}, {65537, 20, 64, 1025, 64, 1025, 257, 256}};

// no part empty: (parts - 1) rows < n <= parts rows
static void require_cover(int64_t n, int64_t rows, int parts, const char* what) {
  REQUIRE(parts >= 1 && rows >= 1, "%s: %d parts of %lld rows", what, parts, (long long)rows);
  REQUIRE((parts - 1) * rows < n && n <= parts * rows, "%s: %d parts of %lld rows, n = %lld", what, parts, (long long)rows, (long long)n);
}

struct Want { const char* name; PsiRegion r; size_t doubles; bool asked; };      // doubles: the largest index its kernels form, + 1
static void require_layout(const PsiPlan& P, const std::vector<Want>& regions) {
  size_t sum = 0;
  for (size_t i = 0; i < regions.size(); ++i) {
    const Want& w = regions[i];
    REQUIRE(w.r.off % 256 == 0, "%s at %zu", w.name, w.r.off);
    REQUIRE(w.asked ? w.r.bytes >= w.doubles * 8 : w.r.bytes == 0, "%s: %zu bytes, %zu doubles %s", w.name, w.r.bytes, w.doubles,
            w.asked ? "needed" : "not asked for");
    REQUIRE(w.r.off <= P.total && w.r.bytes <= P.total - w.r.off, "%s [%zu, + %zu) outside [0, %zu)", w.name, w.r.off, w.r.bytes, P.total);
    for (size_t j = 0; j < i; ++j) {
      const PsiRegion &a = regions[j].r, &b = w.r;
      REQUIRE(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off, "%s and %s overlap", regions[j].name, w.name);
    }
    REQUIRE(sum + w.r.bytes >= sum, "the sum of the sizes wraps at %s", w.name);
    sum += w.r.bytes;
  }
  REQUIRE(P.total >= sum && P.total - sum < 256 * regions.size(), "total %zu, regions %zu: the total wrapped or is not the padded sum", P.total, sum);
}

int main() {
  for (const Row& t : TABLE) {
    g_call = "table row", g_n = t.n, g_M = t.M, g_D = 3, g_asked = 7;
    const PsiPlan f = psi_plan_forward(t.n, t.M, 3, true), g = psi_plan_reverse(t.n, t.M, 3, true, true, true);
    REQUIRE(f.rows_per_split == t.f_rows && f.nsplit == t.f_ns, "forward %lld, %d", (long long)f.rows_per_split, f.nsplit);
    REQUIRE(g.g_rows_per_split == t.g_rows && g.g_nsplit == t.g_ns, "reverse %lld, %d", (long long)g.g_rows_per_split, g.g_nsplit);
    REQUIRE(g.rows_per_chunk == t.z_rows && g.nchunk == t.z_nc, "chunks %lld, %d", (long long)g.rows_per_chunk, g.nchunk);
  }
  std::vector<int64_t> ns;
  for (int64_t n = 1; n <= 3000; ++n) ns.push_back(n);
  for (int64_t n : {40000LL, 45000LL, 65536LL, 65537LL, 1000000LL, 2147483647LL}) ns.push_back(n);
  const int Ms[] = {1, 16, 17, 33, 50, 128, 256, 1000, 2048}, Ds[] = {1, 3, 4, 5, 30, 32, 65};
  long cases = 0;
  for (int64_t n : ns) for (int M : Ms) for (int D : Ds) {
    const size_t N = (size_t)n, nD = N * D, nM = N * M, MD = (size_t)M * D;
    for (int psi2 = 0; psi2 < 2; ++psi2) {
      g_call = "forward", g_n = n, g_M = M, g_D = D, g_asked = psi2;
      const PsiPlan P = psi_plan_forward(n, M, D, psi2);
      REQUIRE(P.Dq % 4 == 0 && P.Dq >= D && P.Dq < D + 4 && P.nt1 == (M + 15) / 16 && P.ntiles == P.nt1 * (P.nt1 + 1) / 2, "Dq %d nt1 %d ntiles %d",
              P.Dq, P.nt1, P.ntiles);
      REQUIRE(P.rows_per_split % 16 == 0, "rows_per_split %lld", (long long)P.rows_per_split);
      require_cover(n, P.rows_per_split, P.nsplit, "row splits");
      require_layout(P, {{"ls", P.ls, (size_t)D, true}, {"W1", P.W1, nD, true}, {"W2", P.W2, nD, true}, {"T", P.T, N * P.Dq, true},
                         {"H1", P.H1, N, true}, {"H2", P.H2, N, true}, {"L", P.L, nM, psi2 != 0},
                         {"part", P.part, (size_t)P.nsplit * P.ntiles * 256, psi2 != 0}});
      ++cases;
    }
    for (int flags = 0; flags < 8; ++flags) {
      const bool g1 = flags & 1, g2 = flags & 2, dZ = flags & 4;
      g_call = "reverse", g_n = n, g_M = M, g_D = D, g_asked = flags;
      const PsiPlan P = psi_plan_reverse(n, M, D, g1, g2, dZ);
      REQUIRE(P.Dq % 4 == 0 && P.Dq >= D && P.Dq < D + 4 && P.nt1 == (M + 15) / 16, "Dq %d nt1 %d", P.Dq, P.nt1);
      REQUIRE(P.g_rows_per_split % 16 == 0, "rows_per_split %lld", (long long)P.g_rows_per_split);
      require_cover(n, P.g_rows_per_split, P.g_nsplit, "row splits");
      require_cover(n, P.rows_per_chunk, P.nchunk, "row chunks");
      REQUIRE(P.nchunk <= PG_Z_CHUNKS, "%d chunks", P.nchunk);
      require_layout(P, {{"ls", P.ls, (size_t)2 * D, true}, {"W1", P.W1, nD, true}, {"W2", P.W2, nD, true}, {"T", P.T, N * P.Dq, true},
                         {"H1", P.H1, N, true}, {"H2", P.H2, N, true}, {"L", P.L, nM, g2}, {"A", P.A, nM, g1}, {"q", P.q, nM, g2},
                         {"Gs", P.Gs, (size_t)M * M, g2}, {"Ppart", P.Ppart, P.nt1 * nD, g2}, {"Spart", P.Spart, P.g_nsplit * MD, g2 && dZ},
                         {"Zpart", P.Zpart, P.nchunk * MD, dZ}, {"Crow", P.Crow, nD, true}, {"AV", P.AV, N, true}});
      ++cases;
    }
  }
  printf("psi_plan_check: %zu table rows, %ld plans, every invariant holds\n", sizeof TABLE / sizeof TABLE[0], cases);
  return 0;
}
