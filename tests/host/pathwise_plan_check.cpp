// Stand-alone check of the plan of the pathwise draws (csrc/pathwise_plan.hpp) on the CPU: a table of chunk counts as literal numbers,
// then the shapes given on the command line (L M D DO S quintuples: the case table of the tests) and a sweep.  For every plan it walks the
// loops of k_pw_eval exactly as the kernel does — the output sweeps and their chunks of 16, the frequency chunks and the four k-steps of
// their two MFMA tiles, the staged chunks of input dimensions and their k-groups, the Z tiles and the sixteen rows a lane group owns —
// and counts how often every frequency, input dimension, inducing row and output is met: each exactly once per sweep, no staged index
// outside its LDS array.  The LDS bytes are the sum of the arrays and within the limit; the regions of the scratch are aligned, disjoint
// and inside the total; both plans are functions of their arguments alone (neither takes the row count, and the kernel's plan does not
// take the draw count).  Exit 1 with a message on the first violated invariant.  Built and run by tests/test_pathwise_plan_cpu.py
// (system C++ compiler, address + undefined sanitizers).
#include "pathwise_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_L, g_M, g_D, g_DO, g_S;
#define REQUIRE(cond, ...)                                                                                                   \
  do {                                                                                                                       \
    if (!(cond)) {                                                                                                           \
      fprintf(stderr, "pathwise_plan_check: L=%d M=%d D=%d DO=%d S=%d\n  violated: %s\n  ", g_L, g_M, g_D, g_DO, g_S, #cond); \
      fprintf(stderr, __VA_ARGS__);                                                                                          \
      fprintf(stderr, "\n");                                                                                                 \
      exit(1);                                                                                                               \
    }                                                                                                                        \
  } while (0)

struct Row { int L, M, D, DO, freq_chunks, d_chunks, k_groups, out_sweeps, z_tiles; };
static const Row TABLE[] = {{1, 0, 1, 1, 1, 1, 1, 1, 0},        {32, 64, 16, 32, 1, 1, 4, 1, 1},     {33, 65, 17, 33, 2, 2, 5, 2, 2},
                            {1024, 128, 8, 8, 32, 1, 2, 1, 2},  {130, 130, 784, 17, 5, 49, 196, 1, 3}, {65536, 2048, 3, 100, 2048, 1, 1, 4, 32}};

static void check(int L, int M, int D, int DO, int S) {
  g_L = L, g_M = M, g_D = D, g_DO = DO, g_S = S;
  const PWPlan P = pathwise_plan(L, M, D, DO);
  const PWPlan Q = pathwise_plan(L, M, D, DO);
  REQUIRE(memcmp(&P, &Q, sizeof P) == 0, "two plans of the same arguments differ");
  REQUIRE(P.lds_bytes == P.lds_x + P.lds_org + P.lds_omega + P.lds_w + P.lds_z + P.lds_ils && P.lds_bytes <= PW_LDS_LIMIT, "LDS %zu",
          P.lds_bytes);
  REQUIRE(P.lds_bytes == pathwise_plan(1, 0, 1, 1).lds_bytes, "the LDS arrays are static: %zu", P.lds_bytes);
  const size_t nx = P.lds_x / 8, nom = P.lds_omega / 8, nw = P.lds_w / 8, nz = P.lds_z / 8;
  std::vector<int> outs(DO, 0);
  int sweeps = 0;
  for (int o0 = 0; o0 < DO; o0 += PW_OC * PW_OG, ++sweeps) {
    for (int q = 0; q < PW_OG; ++q)
      if (o0 + q * PW_OC < DO)
        for (int g = 0; g < 4; ++g)
          for (int t = 0; t < 4; ++t)
            if (o0 + q * PW_OC + g + 4 * t < DO) outs[o0 + q * PW_OC + g + 4 * t] += 1;
    // the prior part
    std::vector<int> freq(L, 0);
    int chunks = 0;
    for (int j0 = 0; j0 < L; j0 += PW_LC, ++chunks) {
      std::vector<int> dims(D, 0);
      int dchunks = 0, groups = 0;
      for (int d0 = 0; d0 < D; d0 += PW_DC, ++dchunks) {
        const int kmax = D - d0 < PW_DC ? D - d0 : PW_DC;
        for (int k = 0; k < kmax; k += 4, ++groups)
          for (int g = 0; g < 4; ++g) {
            REQUIRE((size_t)((PW_RT - 1) * PW_XLD + k + g) < nx && k + g < PW_DC, "x operand at dimension %d", d0 + k + g);
            REQUIRE((size_t)((k + g) * PW_OLD + (PW_LC / 16 - 1) * 16 + 15) < nom, "Omega operand at dimension %d", d0 + k + g);
            if (d0 + k + g < D) dims[d0 + k + g] += 1;
          }
      }
      REQUIRE(dchunks == P.d_chunks && groups == P.k_groups, "%d chunks, %d k-groups", dchunks, groups);
      for (int d = 0; d < D; ++d) REQUIRE(dims[d] == 1, "dimension %d met %d times", d, dims[d]);
      for (int jt = 0; jt < PW_LC / 16; ++jt)
        for (int t = 0; t < 4; ++t)
          for (int g = 0; g < 4; ++g) {
            const int jj = jt * 16 + 4 * t + g;
            REQUIRE((size_t)((PW_LC + jj) * PW_WLD + (PW_OG - 1) * PW_OC + 15) < nw, "weight operand of frequency %d", j0 + jj);
            if (j0 + jj < L) freq[j0 + jj] += 1;
          }
    }
    REQUIRE(chunks == P.freq_chunks, "%d frequency chunks", chunks);
    for (int j = 0; j < L; ++j) REQUIRE(freq[j] == 1, "frequency %d met %d times", j, freq[j]);
    // the update
    std::vector<int> rows(M, 0);
    int tiles = 0;
    for (int m0 = 0; m0 < M; m0 += PW_ZT, ++tiles)
      for (int u = 0; u < PW_ZT / 4; ++u)
        for (int g = 0; g < 4; ++g) {
          REQUIRE((size_t)((4 * u + g) * PW_XLD + PW_DC - 1) < nz, "Z operand of row %d", m0 + 4 * u + g);
          REQUIRE((size_t)((4 * u + g) * PW_WLD + (PW_OG - 1) * PW_OC + 15) < nw, "V operand of row %d", m0 + 4 * u + g);
          if (m0 + 4 * u + g < M) rows[m0 + 4 * u + g] += 1;
        }
    REQUIRE(tiles == P.z_tiles, "%d Z tiles", tiles);
    for (int m = 0; m < M; ++m) REQUIRE(rows[m] == 1, "inducing row %d met %d times", m, rows[m]);
  }
  REQUIRE(sweeps == P.out_sweeps, "%d sweeps", sweeps);
  for (int o = 0; o < DO; ++o) REQUIRE(outs[o] == 1, "output %d written %d times", o, outs[o]);
  // the staging loops cover their arrays in whole passes of the workgroup
  REQUIRE(PW_RT * PW_DC % PW_T == 0 && PW_DC * PW_LC % PW_T == 0 && 2 * PW_LC * PW_OC * PW_OG % PW_T == 0 && PW_ZT * PW_DC % PW_T == 0 &&
              PW_ZT * PW_OC * PW_OG % PW_T == 0 && PW_LC % 16 == 0 && PW_ZT % 4 == 0 && PW_DC % 4 == 0 && PW_RT == PW_T / 64 * 16,
          "tile constants");
  if (M < 1) return;
  const PWScratch A = pathwise_scratch(M, D, DO, S), B = pathwise_scratch(M, D, DO, S);
  REQUIRE(memcmp(&A, &B, sizeof A) == 0, "two carve-ups of the same arguments differ");
  const size_t wide = (size_t)M * S * DO;
  const struct { const char* name; PWRegion r; size_t doubles; } regions[] = {
      {"Zc", A.Zc, (size_t)M * D}, {"Ku", A.Ku, (size_t)M * M}, {"U", A.U, wide}, {"LU", A.LU, wide}, {"F0", A.F0, wide}};
  size_t sum = 0;
  for (size_t i = 0; i < 5; ++i) {
    const PWRegion& r = regions[i].r;
    REQUIRE(r.off % 256 == 0, "%s at %zu", regions[i].name, r.off);
    REQUIRE(r.bytes == regions[i].doubles * 8 && r.bytes > 0, "%s: %zu bytes", regions[i].name, r.bytes);
    REQUIRE(r.off <= A.total && r.bytes <= A.total - r.off, "%s outside the total %zu", regions[i].name, A.total);
    for (size_t j = 0; j < i; ++j)
      REQUIRE(regions[j].r.off + regions[j].r.bytes <= r.off || r.off + r.bytes <= regions[j].r.off, "%s and %s overlap", regions[j].name,
              regions[i].name);
    sum += r.bytes;
  }
  REQUIRE(A.total >= sum && A.total - sum < 256 * 5, "total %zu, regions %zu", A.total, sum);
}

int main(int argc, char** argv) {
  for (const Row& r : TABLE) {
    g_L = r.L, g_M = r.M, g_D = r.D, g_DO = r.DO, g_S = 1;
    const PWPlan P = pathwise_plan(r.L, r.M, r.D, r.DO);
    REQUIRE(P.freq_chunks == r.freq_chunks && P.d_chunks == r.d_chunks && P.k_groups == r.k_groups && P.out_sweeps == r.out_sweeps &&
                P.z_tiles == r.z_tiles,
            "plan (%d, %d, %d, %d, %d)", P.freq_chunks, P.d_chunks, P.k_groups, P.out_sweeps, P.z_tiles);
    check(r.L, r.M, r.D, r.DO, 3);
  }
  if ((argc - 1) % 5 != 0) {
    fprintf(stderr, "usage: pathwise_plan_check [L M D DO S]...\n");
    return 2;
  }
  for (int i = 1; i + 4 < argc; i += 5) check(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]));
  const int Ls[] = {1, 15, 16, 17, 31, 32, 33, 130, 1024}, Ms[] = {0, 1, 17, 63, 64, 65, 130, 2048}, Ds[] = {1, 3, 4, 5, 9, 16, 17, 33, 100, 784},
            DOs[] = {1, 3, 16, 17, 32, 33, 65};
  for (int L : Ls)
    for (int M : Ms)
      for (int D : Ds)
        for (int DO : DOs) check(L, M, D, DO, 1 + (L + M + D + DO) % 5);
  printf("pathwise_plan_check: every invariant holds\n");
  return 0;
}
