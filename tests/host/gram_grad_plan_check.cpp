// Stand-alone check of the plan of the reverse pass of the Gram matrix (csrc/gram_grad_plan.hpp) on the CPU: a table of row blocks and
// column splits as literal numbers, then the shapes given on the command line (n n2 D triples: the case table of the tests) and a sweep
// of n, n2 <= 300 in both forms.  For every plan it walks the launch exactly as k_gg_pass does — workgroup (b, s), thread t, the tiles of
// GG_CT columns of split s — and counts how often every (row, column) pair is met with a non-zero weight and every partial row is
// written: each exactly once, no index outside its matrix or its region.  Exit 1 with a message on the first violated invariant.  Built
// and run by tests/test_gram_grad_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "gram_grad_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static const char* g_call = "";
static long long g_n, g_n2;
static int g_D, g_sym;
#define REQUIRE(cond, ...)                                                          \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      fprintf(stderr, "gram_grad_plan_check: %s n=%lld n2=%lld D=%d symmetric=%d\n  violated: %s\n  ", g_call, g_n, g_n2, g_D, g_sym, #cond); \
      fprintf(stderr, __VA_ARGS__);                                                 \
      fprintf(stderr, "\n");                                                        \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

struct Row { int64_t n, n2; int a_blocks; int64_t a_cols; int a_ns; int b_blocks; int64_t b_cols; int b_ns; };
static const Row TABLE[] = {
    {1, 1, 1, 16, 1, 1, 16, 1},          {15, 17, 1, 32, 1, 1, 16, 1},         {5, 64, 1, 64, 1, 1, 16, 1},
    {5, 65, 1, 48, 2, 1, 16, 1},         {17, 129, 1, 48, 3, 2, 32, 1},        {129, 65, 2, 48, 2, 1, 48, 3},
    {2048, 2048, 16, 64, 32, 16, 64, 32}, {50000, 300, 391, 160, 2, 3, 304, 165}, {100, 100000, 1, 208, 481, 782, 112, 1}};

struct Want { const char* name; GGRegion r; size_t doubles; bool used; };
static void require_layout(const GGPlan& P, const std::vector<Want>& regions) {
  size_t sum = 0;
  for (size_t i = 0; i < regions.size(); ++i) {
    const Want& w = regions[i];
    REQUIRE(w.r.off % 256 == 0, "%s at %zu", w.name, w.r.off);
    REQUIRE(w.used ? w.r.bytes >= w.doubles * 8 : w.r.bytes == 0, "%s: %zu bytes, %zu doubles %s", w.name, w.r.bytes, w.doubles,
            w.used ? "needed" : "not used");
    REQUIRE(w.r.off <= P.total && w.r.bytes <= P.total - w.r.off, "%s [%zu, + %zu) outside [0, %zu)", w.name, w.r.off, w.r.bytes, P.total);
    for (size_t j = 0; j < i; ++j) {
      const GGRegion &a = regions[j].r, &b = w.r;
      REQUIRE(a.bytes == 0 || b.bytes == 0 || a.off + a.bytes <= b.off || b.off + b.bytes <= a.off, "%s and %s overlap", regions[j].name, w.name);
    }
    sum += w.r.bytes;
  }
  REQUIRE(P.total >= sum && P.total - sum < 256 * regions.size(), "total %zu, regions %zu", P.total, sum);
}

// the pass as k_gg_pass walks it: every (row, column) pair once, every partial row once, every index inside
static void walk_pass(const GGPass& p, int D, bool full_walk) {
  REQUIRE(p.row_blocks >= 1 && p.nsplit >= 1 && p.cols_per_split >= GG_CT && p.cols_per_split % GG_CT == 0, "%d blocks, %d splits of %lld",
          p.row_blocks, p.nsplit, (long long)p.cols_per_split);
  REQUIRE((int64_t)(p.row_blocks - 1) * GG_T < p.rows && p.rows <= (int64_t)p.row_blocks * GG_T, "row blocks %d, rows %lld", p.row_blocks,
          (long long)p.rows);
  REQUIRE((p.nsplit - 1) * p.cols_per_split < p.cols && p.cols <= p.nsplit * p.cols_per_split, "%d splits of %lld, cols %lld", p.nsplit,
          (long long)p.cols_per_split, (long long)p.cols);
  REQUIRE(p.nsplit == 1 || p.cols > GG_MIN_COLS, "%d splits of %lld columns", p.nsplit, (long long)p.cols);
  REQUIRE((int64_t)p.row_blocks * p.nsplit <= GG_TARGET_WG + p.row_blocks, "%d x %d workgroups", p.row_blocks, p.nsplit);
  REQUIRE(p.PX.bytes >= (size_t)p.nsplit * p.rows * D * 8, "PX %zu bytes", p.PX.bytes);
  if (!full_walk) return;
  std::vector<int> met((size_t)p.rows * p.cols, 0), written((size_t)p.nsplit * p.rows, 0);
  for (int b = 0; b < p.row_blocks; ++b)
    for (int s = 0; s < p.nsplit; ++s)
      for (int t = 0; t < GG_T; ++t) {
        const int64_t row = (int64_t)b * GG_T + t, rc = row < p.rows ? row : p.rows - 1;
        const int64_t c_lo = (int64_t)s * p.cols_per_split, c_hi = std::min(c_lo + p.cols_per_split, p.cols);
        REQUIRE(c_lo < c_hi, "empty split %d", s);
        for (int64_t c0 = c_lo; c0 < c_hi; c0 += GG_CT)
          for (int cc = 0; cc < GG_CT; ++cc) {
            const int64_t c = c0 + cc, ccl = c < p.cols ? c : p.cols - 1;
            const int staged = c < p.cols ? cc : (int)(p.cols - 1 - c0);
            REQUIRE(staged >= 0 && staged < GG_CT && c0 + staged < p.cols, "staged column %d of tile %lld", staged, (long long)c0);
            REQUIRE(ccl >= 0 && ccl < p.cols && rc >= 0 && rc < p.rows, "clamped indices %lld, %lld", (long long)rc, (long long)ccl);
            if (c < c_hi && row < p.rows) ++met[(size_t)row * p.cols + c];
          }
        if (row < p.rows) {
          const size_t o = (size_t)s * p.rows + row;
          REQUIRE((o + 1) * D * 8 <= p.PX.bytes, "partial row %zu outside PX", o);
          ++written[o];
        }
      }
  for (size_t e = 0; e < met.size(); ++e) REQUIRE(met[e] == 1, "pair (%zu, %zu) met %d times", e / p.cols, e % p.cols, met[e]);
  for (size_t e = 0; e < written.size(); ++e) REQUIRE(written[e] == 1, "partial row %zu written %d times", e, written[e]);
}

static long check(int64_t n, int64_t n2, int D, bool sym, bool full_walk) {
  g_n = n, g_n2 = n2, g_D = D, g_sym = sym;
  const GGPlan P = gram_grad_plan(n, n2, D, sym);
  REQUIRE(P.a.rows == n && P.a.cols == (sym ? n : n2), "pass a %lld x %lld", (long long)P.a.rows, (long long)P.a.cols);
  walk_pass(P.a, D, full_walk);
  if (sym) {
    REQUIRE(P.b.rows == 0 && P.b.PX.bytes == 0, "pass b in the symmetric form");
  } else {
    REQUIRE(P.b.rows == n2 && P.b.cols == n, "pass b %lld x %lld", (long long)P.b.rows, (long long)P.b.cols);
    walk_pass(P.b, D, full_walk);
  }
  const size_t nd = (size_t)n * D, ns = (size_t)P.a.nsplit;
  require_layout(P, {{"PX", P.a.PX, ns * nd, true}, {"PL", P.PL, ns * nd, true}, {"PV", P.PV, ns * n, true}, {"Lrow", P.Lrow, nd, true},
                     {"Vrow", P.Vrow, (size_t)n, true}, {"PX2", P.b.PX, sym ? 0 : (size_t)P.b.nsplit * n2 * D, !sym}});
  // the plan is a function of (n, n2, D, form) alone, and the symmetric form ignores n2
  const GGPlan Q = gram_grad_plan(n, sym ? n2 + 7 : n2, D, sym);
  REQUIRE(Q.total == P.total && Q.a.nsplit == P.a.nsplit && Q.a.cols_per_split == P.a.cols_per_split && Q.b.nsplit == P.b.nsplit,
          "the plan is not reproducible");
  return 1;
}

int main(int argc, char** argv) {
  g_call = "table row";
  for (const Row& t : TABLE) {
    g_n = t.n, g_n2 = t.n2, g_D = 3, g_sym = 0;
    const GGPlan P = gram_grad_plan(t.n, t.n2, 3, false);
    REQUIRE(P.a.row_blocks == t.a_blocks && P.a.cols_per_split == t.a_cols && P.a.nsplit == t.a_ns, "pass a: %d blocks, %d splits of %lld",
            P.a.row_blocks, P.a.nsplit, (long long)P.a.cols_per_split);
    REQUIRE(P.b.row_blocks == t.b_blocks && P.b.cols_per_split == t.b_cols && P.b.nsplit == t.b_ns, "pass b: %d blocks, %d splits of %lld",
            P.b.row_blocks, P.b.nsplit, (long long)P.b.cols_per_split);
  }
  long cases = 0;
  g_call = "case table";
  if ((argc - 1) % 3 != 0) {
    fprintf(stderr, "usage: gram_grad_plan_check [n n2 D]...   (n2 = 0: the symmetric form)\n");
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3) {
    const int64_t n = atoll(argv[a]), n2 = atoll(argv[a + 1]);
    cases += check(n, n2 ? n2 : n, atoi(argv[a + 2]), n2 == 0, true);
  }
  g_call = "sweep";
  for (int64_t n = 1; n <= 300; ++n) {
    cases += check(n, n, 3, true, true);
    // (the pair-by-pair walk for one shape in 31: the invariants on blocks and splits, which imply it, for every one)
    for (int64_t n2 = 1; n2 <= 300; ++n2) cases += check(n, n2, n % 2 ? 1 : 32, false, (n + n2) % 31 == 0);
  }
  g_call = "large";
  for (int64_t n : {2048LL, 50000LL, 1000000LL, 2147483647LL})
    for (int64_t n2 : {1LL, 2048LL, 100000LL, 2147483647LL})
      for (int D : {1, 32}) cases += check(n, n2, D, false, false) + check(n, n2, D, true, false);
  printf("gram_grad_plan_check: %zu table rows, %ld plans, every invariant holds\n", sizeof TABLE / sizeof TABLE[0], cases);
  return 0;
}
