// Stand-alone check of the plan of a stack of sparse sampled layers (csrc/sgpmc_stack_plan.hpp) on the CPU: the shapes given on the
// command line (per stack: L n S DY, then M D DO p per layer — the case table of the tests), a table held to literal numbers and a sweep.
// For every plan, forward-only and with the reverse's regions: the regions of the scratch are aligned, disjoint, large enough and inside
// the total, the forward's regions inside the forward's block; the shared block of the sparse conditional holds every layer's own plan;
// the launches of k_stack_hop (one thread per entry of F), of the per-row kernels and of the read-out's partials are walked as the
// kernels index them and every entry, every row and every partial slot is met exactly once; shapes that do not chain are refused; and
// the plan is a function of its arguments alone.  Exit 1 with a message on the first violated invariant.  Built and run by
// tests/test_sgpmc_stack_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "sgpmc_stack_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

static std::string g_what;
#define REQUIRE(cond, ...)                                                                        \
  do {                                                                                            \
    if (!(cond)) {                                                                                \
      fprintf(stderr, "sgpmc_stack_plan_check: %s\n  violated: %s\n  ", g_what.c_str(), #cond);   \
      fprintf(stderr, __VA_ARGS__);                                                               \
      fprintf(stderr, "\n");                                                                      \
      exit(1);                                                                                    \
    }                                                                                             \
  } while (0)

struct Want { std::string name; SCRegion r; size_t doubles; bool fwd; };

static void require_layout(const StackPlan& P, const std::vector<Want>& regions) {
  size_t sum = 0;
  for (size_t i = 0; i < regions.size(); ++i) {
    const Want& w = regions[i];
    REQUIRE(w.r.off % 256 == 0, "%s at %zu", w.name.c_str(), w.r.off);
    REQUIRE(w.r.bytes >= w.doubles * 8, "%s: %zu bytes, %zu doubles needed", w.name.c_str(), w.r.bytes, w.doubles);
    REQUIRE(w.r.off <= P.total && w.r.bytes <= P.total - w.r.off, "%s [%zu, + %zu) outside [0, %zu)", w.name.c_str(), w.r.off, w.r.bytes,
            P.total);
    if (w.fwd) REQUIRE(w.r.off + w.r.bytes <= P.fwd_total, "%s is not inside the forward's block of %zu", w.name.c_str(), P.fwd_total);
    else REQUIRE(w.r.off >= P.fwd_total, "%s overlaps the forward's block", w.name.c_str());
    for (size_t j = 0; j < i; ++j) {
      const SCRegion &a = regions[j].r, &b = w.r;
      REQUIRE(a.bytes == 0 || b.bytes == 0 || a.off + a.bytes <= b.off || b.off + b.bytes <= a.off, "%s and %s overlap",
              regions[j].name.c_str(), w.name.c_str());
    }
    sum += w.r.bytes;
  }
  REQUIRE(P.total >= sum && P.total - sum < 256 * regions.size(), "total %zu, regions %zu", P.total, sum);
}

// every field of a plan, in order (no memcmp: the struct has padding)
static std::vector<long long> fields(const StackPlan& P) {
  std::vector<long long> f = {P.L, (long long)P.n, (long long)P.R, P.S, P.DY, P.maxM, P.maxD, P.maxDin, P.maxDO, P.ok, (long long)P.sc_bytes,
                              P.head_blocks, (long long)P.fwd_total, (long long)P.total, (long long)P.row_blocks};
  auto reg = [&](const SCRegion& r) { f.push_back((long long)r.off), f.push_back((long long)r.bytes); };
  for (const SCRegion* r : {&P.Zc, &P.Ku, &P.lin, &P.fmean, &P.sc, &P.varb, &P.part, &P.ve, &P.dmean, &P.dvar, &P.prior, &P.gm, &P.gv, &P.dX[0],
                            &P.dX[1]})
    reg(*r);
  for (int l = 0; l < STK_MAX_L; ++l) reg(P.Xin[l]), reg(P.cm[l]), reg(P.var[l]), reg(P.z[l]), f.push_back((long long)P.hop_blocks[l]);
  return f;
}
static bool same(const StackPlan& a, const StackPlan& b) { return fields(a) == fields(b); }

static void check(const StackShape& s, bool walk) {
  char buf[512];
  int at = snprintf(buf, sizeof buf, "L=%d n=%lld S=%d DY=%d", s.L, (long long)s.n, s.S, s.DY);
  for (int l = 0; l < s.L && at < 450; ++l) at += snprintf(buf + at, sizeof buf - at, " [M=%d D=%d DO=%d p=%d]", s.M[l], s.D[l], s.DO[l], s.p[l]);
  g_what = buf;
  for (int reverse = 0; reverse < 2; ++reverse) {
    const StackPlan P = sgpmc_stack_plan(s, reverse != 0);
    StackShape t = s;                                            // what lies past the L layers is not read
    for (int l = s.L; l < STK_MAX_L; ++l) t.M[l] = t.D[l] = t.DO[l] = t.p[l] = 12345;
    const StackPlan Q = sgpmc_stack_plan(t, reverse != 0);
    REQUIRE(P.ok, "the shapes chain, the plan refuses them");
    REQUIRE(same(P, Q), "the plan depends on something besides its arguments");
    const size_t R = (size_t)s.S * (size_t)s.n;
    REQUIRE((size_t)P.R == R && P.L == s.L, "R %lld", (long long)P.R);
    std::vector<Want> w;
    int maxM = 0, maxD = 0, maxDO = 0, maxDin = 1;
    size_t sc = 0;
    for (int l = 0; l < s.L; ++l) {
      maxM = std::max(maxM, s.M[l]), maxD = std::max(maxD, s.D[l]), maxDO = std::max(maxDO, s.DO[l]);
      if (l) maxDin = std::max(maxDin, s.D[l]);
      const SCPlan c = sparse_cond_plan((int64_t)R, s.M[l], s.D[l], s.DO[l]);
      sc = std::max(sc, reverse ? c.total : c.fwd_total);
    }
    REQUIRE(P.sc_bytes == sc, "the shared block of the sparse conditional: %zu, the largest layer needs %zu", P.sc_bytes, sc);
    w.push_back({"Zc", P.Zc, (size_t)maxM * maxD, true});
    w.push_back({"Ku", P.Ku, (size_t)maxM * maxM, true});
    for (int l = 0; l < s.L; ++l) {
      const std::string i = std::to_string(l);
      w.push_back({"Xin" + i, P.Xin[l], R * s.D[l], true});
      w.push_back({"cm" + i, P.cm[l], R * s.DO[l], true});
      w.push_back({"var" + i, P.var[l], R, true});
      w.push_back({"z" + i, P.z[l], l + 1 < s.L ? R * s.DO[l] : 0, true});
      if (l + 1 < s.L) REQUIRE(P.Xin[l + 1].bytes == R * (size_t)(s.p[l] + s.DO[l]) * 8, "the hop of layer %d does not fill the next input", l);
    }
    w.push_back({"lin", P.lin, R * maxDO, true});
    w.push_back({"fmean", P.fmean, R * s.DY, true});
    w.push_back({"sc", P.sc, sc / 8, true});
    w.push_back({"varb", P.varb, R * s.DY, true});
    w.push_back({"part", P.part, (size_t)2 * P.head_blocks, true});
    w.push_back({"ve", P.ve, R, true});
    w.push_back({"dmean", P.dmean, R * s.DY, true});
    w.push_back({"dvar", P.dvar, R * s.DY, true});
    w.push_back({"prior", P.prior, (size_t)s.L, true});
    if (reverse) {
      w.push_back({"gm", P.gm, R * maxDO, false});
      w.push_back({"gv", P.gv, R, false});
      w.push_back({"dX0", P.dX[0], R * maxDin, false});
      w.push_back({"dX1", P.dX[1], R * maxDin, false});
    } else {
      REQUIRE(P.total == P.fwd_total, "a forward-only plan with a reverse block");
    }
    require_layout(P, w);
    // the geometry: blocks of STK_T threads, thread e = block * STK_T + tid, guarded by e < count
    REQUIRE((size_t)P.head_blocks == (R * s.DY + 255) / 256 && P.head_blocks >= 1, "head blocks %d", P.head_blocks);
    REQUIRE((size_t)P.row_blocks == (R + STK_T - 1) / STK_T, "row blocks %lld", (long long)P.row_blocks);
    for (int l = 0; l < s.L; ++l)
      REQUIRE((size_t)P.hop_blocks[l] == (R * (size_t)(s.p[l] + s.DO[l]) + STK_T - 1) / STK_T, "hop blocks of layer %d", l);
    if (!walk) continue;
    for (int l = 0; l < s.L; ++l) {                              // k_stack_hop: entry e -> (r, j); j < p a copy, else output j - p
      const int W = s.p[l] + s.DO[l];
      std::vector<int> F(R * W, 0), Fmean(R * s.DO[l], 0);
      for (int64_t b = 0; b < P.hop_blocks[l]; ++b)
        for (int tid = 0; tid < STK_T; ++tid) {
          const int64_t e = b * STK_T + tid;
          if (e >= (int64_t)(R * W)) continue;
          const int64_t r = e / W;
          const int j = (int)(e - r * W);
          REQUIRE(r >= 0 && (size_t)r < R && j >= 0 && j < W, "entry %lld", (long long)e);
          ++F[(size_t)e];
          if (j >= s.p[l]) ++Fmean[(size_t)r * s.DO[l] + (j - s.p[l])];
        }
      for (int x : F) REQUIRE(x == 1, "an entry of F of layer %d written %d times", l, x);
      for (int x : Fmean) REQUIRE(x == 1, "an entry of Fmean of layer %d written %d times", l, x);
    }
    std::vector<int> rows(R, 0), slots((size_t)2 * P.head_blocks, 0), elems(R * s.DY, 0);
    for (int64_t b = 0; b < P.row_blocks; ++b)
      for (int tid = 0; tid < STK_T; ++tid) {
        const int64_t r = b * STK_T + tid;
        if (r < (int64_t)R) ++rows[(size_t)r];
      }
    for (int x : rows) REQUIRE(x == 1, "a row met %d times", x);
    for (int b = 0; b < P.head_blocks; ++b) {                    // the read-out: block b owns elements [256 b, 256 b + 256) and slots 2 b, 2 b + 1
      ++slots[2 * (size_t)b], ++slots[2 * (size_t)b + 1];
      for (int tid = 0; tid < 256; ++tid) {
        const size_t e = (size_t)b * 256 + tid;
        if (e < R * s.DY) ++elems[e];
      }
    }
    for (int x : slots) REQUIRE(x == 1, "a partial slot written %d times", x);
    for (int x : elems) REQUIRE(x == 1, "an element of the head met %d times", x);
  }
}

static void refuse(StackShape s, const char* why) {
  g_what = why;
  REQUIRE(!sgpmc_stack_plan(s, false).ok && !sgpmc_stack_plan(s, true).ok, "accepted");
}

int main(int argc, char** argv) {
  int stacks = 0;
  for (int i = 1; i < argc;) {
    StackShape s;
    memset(&s, 0, sizeof s);
    if (i + 4 > argc) { fprintf(stderr, "usage: L n S DY {M D DO p} x L ...\n"); return 2; }
    s.L = atoi(argv[i]), s.n = atoll(argv[i + 1]), s.S = atoi(argv[i + 2]), s.DY = atoi(argv[i + 3]);
    i += 4;
    if (s.L < 1 || s.L > STK_MAX_L || i + 4 * s.L > argc) { fprintf(stderr, "bad stack on the command line\n"); return 2; }
    for (int l = 0; l < s.L; ++l, i += 4) s.M[l] = atoi(argv[i]), s.D[l] = atoi(argv[i + 1]), s.DO[l] = atoi(argv[i + 2]), s.p[l] = atoi(argv[i + 3]);
    check(s, true);
    ++stacks;
  }
  // literal numbers: the benchmark shape (3 layers, M = 128, S = 20, minibatch 1000, D = 8)
  {
    StackShape s;
    memset(&s, 0, sizeof s);
    s.L = 3, s.n = 1000, s.S = 20, s.DY = 1;
    for (int l = 0; l < 3; ++l) s.M[l] = 128, s.D[l] = 8, s.DO[l] = l < 2 ? 8 : 1, s.p[l] = 0;
    const StackPlan P = sgpmc_stack_plan(s, true);
    g_what = "the benchmark shape";
    REQUIRE(P.ok && P.R == 20000 && P.head_blocks == 79 && P.row_blocks == 79 && P.hop_blocks[0] == 625 && P.hop_blocks[2] == 79,
            "R %lld head %d rows %lld hop %lld %lld", (long long)P.R, P.head_blocks, (long long)P.row_blocks, (long long)P.hop_blocks[0],
            (long long)P.hop_blocks[2]);
    REQUIRE(P.sc_bytes == sparse_cond_plan(20000, 128, 8, 8).total && P.maxDin == 8 && P.maxDO == 8 && P.maxM == 128, "the shared block");
    check(s, true);
  }
  // a sweep over depths, row counts around the workgroup size, widths and propagated inputs
  const int64_t ns[] = {1, 2, 51, 255, 256, 257, 511, 513, 1000};
  const int widths[] = {1, 3, 16, 17}, Ms[] = {1, 5, 16, 65};
  int swept = 0;
  for (int L = 1; L <= 4; ++L)
    for (int64_t n : ns)
      for (int S : {1, 3})
        for (int v = 0; v < 4; ++v)
          for (int p : {0, 2}) {
            StackShape s;
            memset(&s, 0, sizeof s);
            s.L = L, s.n = n, s.S = S;
            int D = 2 + v;
            for (int l = 0; l < L; ++l) {
              s.M[l] = Ms[(v + l) % 4], s.D[l] = D, s.DO[l] = widths[(v + l) % 4];
              s.p[l] = l + 1 < L ? std::min(p, D) : 0;
              D = s.p[l] + s.DO[l];
            }
            s.DY = s.DO[L - 1];
            check(s, n * S <= 1100);
            ++swept;
          }
  // shapes that do not chain
  {
    StackShape s;
    memset(&s, 0, sizeof s);
    s.L = 2, s.n = 10, s.S = 2, s.DY = 1;
    s.M[0] = s.M[1] = 5, s.D[0] = 3, s.DO[0] = 2, s.p[0] = 1, s.D[1] = 3, s.DO[1] = 1, s.p[1] = 0;
    check(s, true);
    StackShape t = s;
    t.D[1] = 4, refuse(t, "input_dim[1] != p[0] + DO[0]");
    t = s, t.p[1] = 1, refuse(t, "the last layer propagates inputs");
    t = s, t.DY = 2, refuse(t, "DO of the last layer is not the likelihood's width");
    t = s, t.p[0] = 4, refuse(t, "p > D");
    t = s, t.M[0] = SC_MAX_M + 1, refuse(t, "M above the limit");
    t = s, t.L = 0, refuse(t, "no layer");
    t = s, t.L = STK_MAX_L + 1, refuse(t, "too many layers");
    t = s, t.n = (int64_t)1 << 30, t.S = 2, refuse(t, "S n = 2^31");
    t = s, t.n = 0, refuse(t, "no rows");
  }
  printf("sgpmc_stack_plan_check: %d stacks from the command line, %d swept: every invariant holds\n", stacks, swept);
  return 0;
}
