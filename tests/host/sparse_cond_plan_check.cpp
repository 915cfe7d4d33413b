// Stand-alone check of the plan of the sparse conditional without q_sqrt (csrc/sparse_cond_plan.hpp) on the CPU: a table of tiles and
// splits as literal numbers, then the shapes given on the command line (n M D DO quadruples: the case table of the tests) and a sweep.
// For every plan it walks the two launches exactly as k_sc_fwd and k_sc_adj do — the forward's workgroup per tile, the reverse's
// workgroup (split, row chunk), the four waves' rows and columns of the staged block — and counts how often every row of X, every row of
// A, every output and every partial slot is met: each exactly once, no index outside its matrix or its region.  The regions of the
// scratch are aligned, disjoint and inside the total, and the plan is a function of (n, M, D, DO) alone.  Exit 1 with a message on the
// first violated invariant.  Built and run by tests/test_sparse_cond_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "sparse_cond_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static const char* g_call = "";
static long long g_n;
static int g_M, g_D, g_DO;
#define REQUIRE(cond, ...)                                                                                                      \
  do {                                                                                                                          \
    if (!(cond)) {                                                                                                              \
      fprintf(stderr, "sparse_cond_plan_check: %s n=%lld M=%d D=%d DO=%d\n  violated: %s\n  ", g_call, g_n, g_M, g_D, g_DO, #cond); \
      fprintf(stderr, __VA_ARGS__);                                                                                             \
      fprintf(stderr, "\n");                                                                                                    \
      exit(1);                                                                                                                  \
    }                                                                                                                           \
  } while (0)

struct Row { int64_t n; int M, DO; int64_t tiles; int chunks, groups; int64_t tps; int nsplit; };
static const Row TABLE[] = {{1, 1, 1, 1, 1, 1, 1, 1},           {64, 64, 64, 1, 1, 1, 1, 1},          {65, 65, 65, 2, 2, 2, 1, 2},
                            {16384, 3, 1, 256, 1, 1, 1, 256},   {16385, 3, 1, 257, 1, 1, 2, 129},     {40000, 128, 8, 625, 2, 1, 3, 209},
                            {2147483647LL, 2048, 1, 33554432, 32, 1, 131072, 256}};

struct Want { const char* name; SCRegion r; size_t doubles; };
static void require_layout(const SCPlan& P, const std::vector<Want>& regions, size_t fwd_regions) {
  size_t sum = 0;
  for (size_t i = 0; i < regions.size(); ++i) {
    const Want& w = regions[i];
    REQUIRE(w.r.off % 256 == 0, "%s at %zu", w.name, w.r.off);
    REQUIRE(w.r.bytes >= w.doubles * 8 && w.r.bytes > 0, "%s: %zu bytes, %zu doubles needed", w.name, w.r.bytes, w.doubles);
    REQUIRE(w.r.off <= P.total && w.r.bytes <= P.total - w.r.off, "%s [%zu, + %zu) outside [0, %zu)", w.name, w.r.off, w.r.bytes, P.total);
    if (i < fwd_regions) REQUIRE(w.r.off + w.r.bytes <= P.fwd_total, "%s is not inside the forward's block of %zu", w.name, P.fwd_total);
    else REQUIRE(w.r.off >= P.fwd_total, "%s overlaps the forward's block", w.name);
    for (size_t j = 0; j < i; ++j) {
      const SCRegion &a = regions[j].r, &b = w.r;
      REQUIRE(a.off + a.bytes <= b.off || b.off + b.bytes <= a.off, "%s and %s overlap", regions[j].name, w.name);
    }
    sum += w.r.bytes;
  }
  REQUIRE(P.total >= sum && P.total - sum < 256 * regions.size(), "total %zu, regions %zu", P.total, sum);
}

static void walk(const SCPlan& P) {
  const int64_t n = P.n;
  const int M = P.M, DO = P.DO;
  // k_sc_fwd: workgroup = tile; wave w, lane (g, c), register t own mean[r0 + 16 w + g + 4 t][o0 + 16 q + c]; thread tid < SC_CT owns var
  std::vector<int> mean((size_t)n * DO, 0), var((size_t)n, 0), rows_read((size_t)M, 0);
  for (int64_t tile = 0; tile < P.tiles; ++tile) {
    const int64_t r0 = tile * SC_CT;
    REQUIRE(r0 < n, "tile %lld starts past the end", (long long)tile);
    for (int og = 0; og < P.out_groups; ++og)
      for (int w = 0; w < SC_T / 64; ++w)
        for (int g = 0; g < 4; ++g)
          for (int c = 0; c < 16; ++c)
            for (int q = 0; q < SC_DOG; ++q)
              for (int t = 0; t < 4; ++t) {
                const int64_t r = r0 + w * 16 + g + 4 * t;
                const int o = og * SC_DOC * SC_DOG + q * SC_DOC + c;
                if (r < n && o < DO) ++mean[(size_t)r * DO + o];
              }
    for (int tid = 0; tid < SC_CT; ++tid)
      if (r0 + tid < n) ++var[(size_t)(r0 + tid)];
    if (tile == 0)
      for (int i0 = 0; i0 < M; i0 += SC_KC)
        for (int row = 0; row < SC_KC; ++row)
          if (i0 + row < M) ++rows_read[(size_t)(i0 + row)];
  }
  for (size_t e = 0; e < mean.size(); ++e) REQUIRE(mean[e] == 1, "mean entry %zu written %d times", e, mean[e]);
  for (size_t e = 0; e < var.size(); ++e) REQUIRE(var[e] == 1, "var entry %zu written %d times", e, var[e]);
  for (size_t e = 0; e < rows_read.size(); ++e) REQUIRE(rows_read[e] == 1, "row %zu of A read %d times", e, rows_read[e]);
  // k_sc_adj: workgroup (s, chunk): the tiles of split s, the rows of the chunk; A_bar[i][r] once, PW[s][i][o] once, every (i, r) of A gm once
  std::vector<int> abar((size_t)M * n, 0), pw((size_t)P.nsplit * M * DO, 0), tiles_met((size_t)P.tiles, 0);
  for (int s = 0; s < P.nsplit; ++s) {
    const int64_t t_lo = (int64_t)s * P.tiles_per_split, t_hi = std::min(t_lo + P.tiles_per_split, P.tiles);
    REQUIRE(t_lo < t_hi, "empty split %d", s);
    for (int64_t tile = t_lo; tile < t_hi; ++tile) ++tiles_met[(size_t)tile];
    for (int ch = 0; ch < P.row_chunks; ++ch) {
      const int i0 = ch * SC_KC;
      REQUIRE(i0 < M, "chunk %d starts past the end", ch);
      for (int w = 0; w < SC_T / 64; ++w)
        for (int g = 0; g < 4; ++g)
          for (int c = 0; c < 16; ++c)
            for (int t = 0; t < 4; ++t) {
              const int i = i0 + w * 16 + g + 4 * t;
              for (int64_t tile = t_lo; tile < t_hi; ++tile)
                for (int b = 0; b < SC_CT / 16; ++b) {
                  const int64_t r = tile * SC_CT + b * 16 + c;
                  if (i < M && r < n) ++abar[(size_t)i * n + r];
                }
              for (int og = 0; og < P.out_groups; ++og)
                for (int q = 0; q < SC_DOG; ++q) {
                  const int o = og * SC_DOC * SC_DOG + q * SC_DOC + c;
                  if (i < M && o < DO) {
                    const size_t slot = ((size_t)s * M + i) * DO + o;
                    REQUIRE((slot + 1) * 8 <= P.PW.bytes, "partial slot %zu outside PW", slot);
                    ++pw[slot];
                  }
                }
            }
    }
  }
  for (size_t e = 0; e < tiles_met.size(); ++e) REQUIRE(tiles_met[e] == 1, "tile %zu is in %d splits", e, tiles_met[e]);
  for (size_t e = 0; e < abar.size(); ++e) REQUIRE(abar[e] == 1, "A_bar entry %zu written %d times", e, abar[e]);
  for (size_t e = 0; e < pw.size(); ++e) REQUIRE(pw[e] == 1, "partial slot %zu written %d times", e, pw[e]);
}

static long check(int64_t n, int M, int D, int DO, bool full_walk) {
  g_n = n, g_M = M, g_D = D, g_DO = DO;
  const SCPlan P = sparse_cond_plan(n, M, D, DO);
  REQUIRE(P.n == n && P.M == M && P.D == D && P.DO == DO, "the plan does not carry its arguments");
  REQUIRE((P.tiles - 1) * SC_CT < n && n <= P.tiles * SC_CT, "%lld tiles", (long long)P.tiles);
  REQUIRE((P.row_chunks - 1) * SC_KC < M && M <= P.row_chunks * SC_KC, "%d row chunks", P.row_chunks);
  REQUIRE((P.out_groups - 1) * SC_DOC * SC_DOG < DO && DO <= P.out_groups * SC_DOC * SC_DOG, "%d output groups", P.out_groups);
  REQUIRE(P.nsplit >= 1 && P.nsplit <= SC_TARGET_SPLITS && P.tiles_per_split >= 1, "%d splits of %lld tiles", P.nsplit,
          (long long)P.tiles_per_split);
  REQUIRE((P.nsplit - 1) * P.tiles_per_split < P.tiles && P.tiles <= P.nsplit * P.tiles_per_split, "%d splits of %lld tiles, %lld tiles",
          P.nsplit, (long long)P.tiles_per_split, (long long)P.tiles);
  const size_t mm = (size_t)M * M, mn = (size_t)M * (size_t)n, mo = (size_t)M * DO, md = (size_t)M * D;
  require_layout(P, {{"Ku", P.Ku, mm}, {"A", P.A, mn}, {"W", P.W, mo}, {"Zc", P.Zc, md}, {"Xc", P.Xc, (size_t)n * D},
                     {"Abar", P.Abar, mn}, {"PW", P.PW, (size_t)P.nsplit * mo}, {"Wbar", P.Wbar, mo}, {"V", P.V, mo}, {"T", P.T, mm},
                     {"Q", P.Q, mm}, {"S", P.S, mm}, {"St", P.St, mm}, {"dZ1", P.dZ1, md}, {"dZ2", P.dZ2, md},
                     {"dk1", P.dk1, (size_t)2 + D}, {"dk2", P.dk2, (size_t)2 + D}}, 5);
  if (full_walk) walk(P);
  // a function of its four arguments alone: a second evaluation, after other plans were made, is the same plan byte for byte
  (void)sparse_cond_plan(n + 1, M, D, DO);
  const SCPlan Q = sparse_cond_plan(n, M, D, DO);
  const SCRegion pr[] = {P.Ku, P.A, P.W, P.Zc, P.Xc, P.Abar, P.PW, P.Wbar, P.V, P.T, P.Q, P.S, P.St, P.dZ1, P.dZ2, P.dk1, P.dk2};
  const SCRegion qr[] = {Q.Ku, Q.A, Q.W, Q.Zc, Q.Xc, Q.Abar, Q.PW, Q.Wbar, Q.V, Q.T, Q.Q, Q.S, Q.St, Q.dZ1, Q.dZ2, Q.dk1, Q.dk2};
  bool same = Q.tiles == P.tiles && Q.row_chunks == P.row_chunks && Q.out_groups == P.out_groups && Q.tiles_per_split == P.tiles_per_split &&
              Q.nsplit == P.nsplit && Q.fwd_total == P.fwd_total && Q.total == P.total;
  for (size_t i = 0; i < sizeof pr / sizeof pr[0]; ++i) same = same && pr[i].off == qr[i].off && pr[i].bytes == qr[i].bytes;
  REQUIRE(same, "the plan is not reproducible");
  // and the summation order (tiles, splits) does not depend on D
  const SCPlan R = sparse_cond_plan(n, M, D + 1, DO);
  REQUIRE(R.tiles == P.tiles && R.nsplit == P.nsplit && R.tiles_per_split == P.tiles_per_split, "the splits depend on D");
  return 1;
}

int main(int argc, char** argv) {
  g_call = "table row";
  for (const Row& t : TABLE) {
    g_n = t.n, g_M = t.M, g_D = 3, g_DO = t.DO;
    const SCPlan P = sparse_cond_plan(t.n, t.M, 3, t.DO);
    REQUIRE(P.tiles == t.tiles && P.row_chunks == t.chunks && P.out_groups == t.groups && P.tiles_per_split == t.tps && P.nsplit == t.nsplit,
            "%lld tiles, %d chunks, %d groups, %d splits of %lld tiles", (long long)P.tiles, P.row_chunks, P.out_groups, P.nsplit,
            (long long)P.tiles_per_split);
  }
  long cases = 0;
  g_call = "case table";
  if ((argc - 1) % 4 != 0) {
    fprintf(stderr, "usage: sparse_cond_plan_check [n M D DO]...\n");
    return 2;
  }
  for (int a = 1; a + 3 < argc; a += 4) cases += check(atoll(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), true);
  g_call = "sweep";
  for (int64_t n = 1; n <= 200; ++n)
    for (int M : {1, 15, 16, 17, 63, 64, 65, 130})
      cases += check(n, M, 1 + (int)(n % 32), 1 + (int)((n * 7 + M) % 70), (n + M) % 13 == 0);
  for (int64_t n = 16000; n <= 17000; n += 37) cases += check(n, 3, 2, 2, n % 5 == 0);
  g_call = "large";
  for (int64_t n : {40000LL, 1000000LL, 2147483647LL})
    for (int M : {1, 128, 2048})
      for (int DO : {1, 65}) cases += check(n, M, 32, DO, false);
  printf("sparse_cond_plan_check: %zu table rows, %ld plans, every invariant holds\n", sizeof TABLE / sizeof TABLE[0], cases);
  return 0;
}
