// Stand-alone check of the split-K planner (csrc/model_plan.hpp) on the CPU: fake base addresses, a grid of shapes, exit 1 with a
// message on the first violated invariant.  Built and run by tests/test_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "model_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string>

struct Buf { const char* name; uintptr_t lo, hi; };      // [lo, hi) in bytes
static uintptr_t g_top;
static std::string g_case;
template <class T>
static T* fake(Buf& b, const char* name, size_t count) {      // the bump allocator of the workspace layout, on addresses nobody reads
  g_top = (g_top + 255) / 256 * 256;
  b = Buf{name, g_top, g_top + count * sizeof(T)};
  g_top = b.hi;
  return (T*)b.lo;
}
#define REQUIRE(cond, ...)                                                     \
  do {                                                                         \
    if (!(cond)) {                                                             \
      fprintf(stderr, "plan_check: %s\n  violated: %s\n  ", g_case.c_str(), #cond); \
      fprintf(stderr, __VA_ARGS__);                                            \
      fprintf(stderr, "\n");                                                   \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

static int job_tasks(const WgradJob& J, int ns) {
  const int n_off = J.ti * (J.ti - 1) / 2;
  if (J.ng) return 4 * ns * n_off + 3 * J.ns_diag * J.ti;
  return J.sym ? ns * n_off + J.ns_diag * J.ti : ns * J.ti * J.tj;
}
static int red_blocks(const RedJob& r) {      // from the form plan_reductions chose
  const int64_t rows = r.out_ld > 0 ? r.count / r.out_ld : 0;
  if (r.wide) return (int)r.count;
  if (r.ways == 64) return (int)((rows / 64) * (rows / 64 + 1) / 2);
  if (r.ways == 16) return (int)((rows / 16) * (rows / 16 + 1) / 2);
  return ceil_div(r.count, r.ways == 8 ? 128 : (r.ways == 4 ? 64 : 256));
}
struct Span { uintptr_t lo, hi; int job; };
static void require_disjoint(std::vector<Span>& v, const char* what) {
  std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  for (size_t i = 1; i < v.size(); ++i)
    REQUIRE(v[i - 1].hi <= v[i].lo, "%s of jobs %d and %d overlap", what, v[i - 1].job, v[i].job);
}

int main() {
  const int Mps[] = {16, 48, 64, 112, 128, 192, 256, 512, 1024}, Douts[] = {1, 2, 3, 5, 8, 30}, Dins[] = {1, 8, 16, 33, 784};
  const int64_t Rins[] = {16, 100, 2000, 20000, 500000};
  long cases = 0;
  std::vector<RedJob> window[3];      // the reductions of the last three plans: the "layers" of one list for invariant 6
  PlanOut P;
  for (int Mp : Mps) for (int D_out : Douts) for (int D_in : Dins) for (int64_t Rin : Rins)
  for (int alg_g = 0; alg_g < 2; ++alg_g) for (int mean_grad = 0; mean_grad < 2; ++mean_grad) for (int wg_red = 0; wg_red < 3; ++wg_red)
  for (int wg_group = 0; wg_group < 3; ++wg_group) for (int overlap = 0; overlap < 2; ++overlap) for (int roomy = 0; roomy < 2; ++roomy) {
    char txt[256];
    snprintf(txt, sizeof txt, "Mp=%d D_out=%d D_in=%d Rin=%lld alg_g=%d mean_grad=%d wg_red=%d wg_group=%d overlap=%d ld_max=%s", Mp, D_out,
             D_in, (long long)Rin, alg_g, mean_grad, wg_red, wg_group, overlap, roomy ? "3 ld" : "ld");
    g_case = txt;
    g_top = 0x10000000;
    LayerDev v{};
    PlanBufs bufs{};      // (the layer's buffers; the LayerDev carries its shape and results)
    v.Mp = Mp; v.D_out = D_out; v.D_in = D_in; v.DP16 = (int)round_up(D_out, 16); v.DinP16 = (int)round_up(D_in + 1, 16);
    v.alg_g = alg_g; bufs.mean_grad = mean_grad != 0;
    const PlanIn pin{&v, &bufs, round_up(Rin, 16), 32, wg_red, wg_group, overlap};
    const int64_t ld_max = roomy ? 3 * pin.ld : pin.ld, MM = (int64_t)Mp * Mp;
    const int Mw = pad_Mw(Mp), mean_rows = 64 * ceil_div(v.DinP16, 64);
    bufs.cap = plan_caps(alg_g, D_out, Mp, v.DP16, v.DinP16, bufs.mean_grad, ld_max);
    Buf bA, bE, bGW, bVB, bMB, bXT1, bhyp, bbig, bthin, bmean, btick, bbigred, bthinq, bthinz, bmeanAB, bhypred;
    bufs.A = fake<double>(bA, "A", (size_t)Mw * ld_max); bufs.E = fake<double>(bE, "E", (size_t)Mw * ld_max);
    bufs.GW = fake<double>(bGW, "GW", (size_t)Mw * ld_max); bufs.VB = fake<double>(bVB, "VB", (size_t)v.DP16 * ld_max);
    bufs.MB = fake<double>(bMB, "MB", (size_t)v.DP16 * ld_max); bufs.XT1 = fake<double>(bXT1, "XT1", (size_t)mean_rows * ld_max);
    bufs.hyp_part = fake<double>(bhyp, "hyp_part", (size_t)pin.hyp_parts * (D_in + 2));
    bufs.part_big = fake<double>(bbig, "part_big", bufs.cap.part_big); bufs.part_thin = fake<double>(bthin, "part_thin", bufs.cap.part_thin);
    bufs.part_mean = bufs.mean_grad ? fake<double>(bmean, "part_mean", bufs.cap.part_mean) : nullptr;
    bufs.wtick = fake<int32_t>(btick, "wtick", bufs.cap.ticks);
    v.bigred = fake<double>(bbigred, "bigred", (size_t)(1 + D_out) * MM); v.thinq = fake<double>(bthinq, "thinq", (size_t)Mp * v.DP16);
    v.thinz = fake<double>(bthinz, "thinz", (size_t)Mp * v.DinP16);
    v.meanAB = bufs.mean_grad ? fake<double>(bmeanAB, "meanAB", (size_t)mean_rows * v.DP16) : nullptr;
    v.hyp_red = fake<double>(bhypred, "hyp_red", D_in + 2 + 8);
    plan_layer(pin, P);
    const int ns = P.ns, njobs = (int)P.jobs.size();

    // 3. capacities
    REQUIRE(ns >= 1 && ns <= bufs.cap.ns_max, "ns %d, split cap %d", ns, bufs.cap.ns_max);
    REQUIRE(njobs <= bufs.cap.jobs, "%d jobs, %d slots", njobs, bufs.cap.jobs);
    REQUIRE(P.ticks <= bufs.cap.ticks, "%d tickets, %d slots", P.ticks, bufs.cap.ticks);
    REQUIRE((int)P.red.size() <= bufs.cap.reds, "%d reductions, %d slots", (int)P.red.size(), bufs.cap.reds);

    // 1. task ranges tile [0, tot) in list order, the A jobs first and up to totA
    int next = 0;
    REQUIRE(P.njobsA >= 1 && P.njobsA <= njobs, "njobsA %d of %d", P.njobsA, njobs);
    for (int i = 0; i < njobs; ++i) {
      if (i == P.njobsA) REQUIRE(next == P.totA, "A jobs end at task %d, totA %d", next, P.totA);
      REQUIRE(P.jobs[i].task_start == next, "job %d starts at task %d, expected %d", i, P.jobs[i].task_start, next);
      REQUIRE(job_tasks(P.jobs[i], ns) > 0, "job %d has no task", i);
      next += job_tasks(P.jobs[i], ns);
    }
    REQUIRE(next == P.tot && (P.njobsA < njobs || P.totA == P.tot), "tasks end at %d, tot %d, totA %d", next, P.tot, P.totA);

    // 2. partial regions inside their buffers, disjoint; 5. groups; ticket ranges
    std::vector<Span> parts, ticks;
    int grouped = 0, single_pd = 0;
    for (int i = 0; i < njobs; ++i) {
      const WgradJob& J = P.jobs[i];
      const size_t one = (size_t)ns * (J.ti * 64) * J.ldo;      // ns splits (a diagonal tile fills its first ns_diag) x rows x ldo
      REQUIRE(!J.sym || (J.ns_diag >= 1 && J.ns_diag <= ns), "job %d: ns_diag %d, ns %d", i, J.ns_diag, ns);
      REQUIRE(J.ng >= 0 && J.ng <= 4, "job %d: group of %d", i, J.ng);
      if (J.ng) {
        REQUIRE(J.sym && !J.fin && !J.tick, "job %d: a group must be symmetric and leave partials", i);
        REQUIRE((size_t)J.ostride >= one, "job %d: results of the group %lld apart, each %zu", i, (long long)J.ostride, one);
        grouped += J.ng;
      } else if (J.sym) ++single_pd;
      const size_t ext = J.ng ? (size_t)(J.ng - 1) * J.ostride + one : one;
      const uintptr_t lo = (uintptr_t)J.out, hi = lo + ext * sizeof(double);
      const Buf& b = (lo >= bbig.lo && lo < bbig.hi) ? bbig : ((bufs.mean_grad && lo >= bmean.lo && lo < bmean.hi) ? bmean : bthin);
      REQUIRE(lo >= b.lo && hi <= b.hi, "job %d: partials [%#zx, %#zx) outside %s [%#zx, %#zx)", i, (size_t)lo, (size_t)hi, b.name, (size_t)b.lo,
              (size_t)b.hi);
      parts.push_back(Span{lo, hi, i});
      if (J.fin) {
        const uintptr_t tl = (uintptr_t)J.tick, th = tl + (size_t)(J.sym ? J.ti * (J.ti + 1) / 2 : J.ti * J.tj) * sizeof(int32_t);
        REQUIRE(J.tick && tl >= btick.lo && th <= btick.hi, "job %d: tickets outside wtick", i);
        ticks.push_back(Span{tl, th, i});
      }
    }
    require_disjoint(parts, "partial regions");
    require_disjoint(ticks, "ticket ranges");
    REQUIRE((grouped == D_out && single_pd == 0) || (grouped == 0 && single_pd == D_out), "%d grouped + %d single P_d, D_out %d", grouped,
            single_pd, D_out);

    // 4. every result from exactly one of a fin job or a RedJob, and nothing else written
    std::vector<const double*> want, got;
    for (int j = alg_g ? 1 : 0; j <= D_out; ++j) want.push_back(v.bigred + (int64_t)j * MM);
    want.push_back(v.thinq); want.push_back(v.thinz); want.push_back(v.hyp_red);
    if (bufs.mean_grad) want.push_back(v.meanAB);
    for (const WgradJob& J : P.jobs) if (J.fin) got.push_back(J.fin);
    for (const RedJob& r : P.red) got.push_back(r.out);
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    REQUIRE(want == got, "%zu results wanted, %zu produced (or a result produced twice / a stray target)", want.size(), got.size());

    // 6. reduction block ranges: contiguous over a list of three layers, each layer's range exactly its jobs
    window[cases % 3] = P.red;
    std::vector<RedJob> red;
    int off[4] = {0, 0, 0, 0};
    for (int l = 0; l < 3; ++l) {
      red.insert(red.end(), window[l].begin(), window[l].end());
      off[l + 1] = (int)red.size();
    }
    const RedPlan rp = plan_reductions(red);
    auto blk_at = [&](int idx) { return idx < (int)red.size() ? red[idx].blk_start : rp.blocks; };      // first block of job idx (the end for idx = size)
    int blk = 0;
    bool any64 = false;
    for (size_t i = 0; i < red.size(); ++i) {
      REQUIRE(red[i].blk_start == blk && red_blocks(red[i]) > 0, "reduction %zu starts at block %d, expected %d", i, red[i].blk_start, blk);
      blk += red_blocks(red[i]);
      any64 = any64 || red[i].ways == 64;
    }
    REQUIRE(blk == rp.blocks && any64 == rp.any64, "%d blocks counted, %d planned", blk, rp.blocks);
    for (int l = 0; l < 3; ++l) {
      int sum = 0;
      for (int i = off[l]; i < off[l + 1]; ++i) sum += red_blocks(red[i]);
      REQUIRE(blk_at(off[l + 1]) - blk_at(off[l]) == sum, "layer %d: range of %d blocks, its jobs have %d", l,
              blk_at(off[l + 1]) - blk_at(off[l]), sum);
    }
    REQUIRE(blk_at(0) == 0 && blk_at(off[3]) == rp.blocks, "the list's range is not [0, %d)", rp.blocks);
    ++cases;
  }
  printf("plan_check: %ld plans, every invariant holds\n", cases);
  return 0;
}
