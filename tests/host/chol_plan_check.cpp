// Stand-alone check of the plan of the blocked Cholesky + triangular inverse (csrc/chol_plan.hpp) on the CPU.  Built and run by
// tests/test_chol_plan_cpu.py (system C++ compiler, address + undefined sanitizers).  For n = 128 .. 2304 in steps of 64, five real
// orders, four batch sizes and every legal flag combination it REPLAYS the plan's steps against the algorithm, not against the planner's
// arithmetic: the matrix as 64 x 64 tiles, every lower tile recording which panels' updates it has received, whether its L is final and
// where it sits (parked transposed above the block diagonal, or in place), every block of the inverse recording the terms it summed.
// The side tasks are decoded as the kernels decode them (chol_wide_update, chol_xrow, k_chol_panel of linalg.hip).  Exit 1 with a
// message on the first violated invariant; prints the number of (input, invariant) checks made.
//
// PINNED below: the full step lists of six inputs, written by hand from the parent commit's bigchol_build and bigchol_run (the code this
// planner replaced), NOT from the planner's output.
#include "chol_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

static std::string g_what;
static long g_checks = 0;
#define REQUIRE(cond, ...)                                                                   \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      fprintf(stderr, "chol_plan_check: %s\n  violated: %s\n  ", g_what.c_str(), #cond);     \
      fprintf(stderr, __VA_ARGS__);                                                          \
      fprintf(stderr, "\n");                                                                 \
      exit(1);                                                                               \
    }                                                                                        \
  } while (0)

static std::string describe(const CholIn& in) {
  char b[200];
  snprintf(b, sizeof b, "n=%d nreal=%d batch=%d inverse=%d transpose=%d from_tri=%d need_factor=%d caller_tbuf=%d lookahead_allowed=%d", in.n,
           in.nreal, in.batch, in.want_inverse, in.want_transpose, in.from_tri, in.need_factor, in.caller_tbuf, in.lookahead_allowed);
  return b;
}
static std::string show(const CholStep& s) {
  char b[200];
  switch (s.kind) {
    case CS_BLOCK: snprintf(b, sizeof b, "B q=%d g=%d w=%d xa=%d/%d/%d xb=%d/%d/%d s=%d", s.q, s.gx, s.nwide, s.xa.i, s.xa.nx, s.xa.mode, s.xb.i, s.xb.nx, s.xb.mode, s.side); break;
    case CS_PANEL: snprintf(b, sizeof b, "P p=%d g=%dx%d", s.q, s.gx, s.gy); break;
    case CS_GEMM: snprintf(b, sizeof b, "G f=%d c=%d big=%d g=%d", s.first, s.count, s.allow_big, s.gx); break;
    case CS_XROW_LAST: snprintf(b, sizeof b, "X i=%d nx=%d m=%d g=%d", s.xa.i, s.xa.nx, s.xa.mode, s.gx); break;
    case CS_TRTRI_DIAG64: snprintf(b, sizeof b, "T g=%d", s.gx); break;
    case CS_MIRROR: snprintf(b, sizeof b, "M g=%dx%d", s.gx, s.gy); break;
    case CS_TRANSPOSE: snprintf(b, sizeof b, "Tr g=%dx%d", s.gx, s.gy); break;
    default: snprintf(b, sizeof b, "? kind %d", s.kind);
  }
  return b;
}

// ------------------------------------------------------------------------------------------------ the legal calls, listed
//                                 inverse transpose from_tri need_factor caller_tbuf
static const bool LEGAL[][5] = {{0, 0, 0, 1, 0},      // factor only (dsdgp_potrf)
                                {0, 0, 0, 1, 1},      //   ... the caller lends Tbuf
                                {1, 0, 0, 1, 0},      // factor + inverse
                                {1, 1, 0, 1, 0},      //   ... + its transpose (Ku of a white = True model)
                                {1, 0, 0, 0, 0},      // inverse and log det only
                                {1, 1, 0, 0, 0},      //   ... (Ku of a white = False model, A of the natural-gradient step)
                                {1, 0, 1, 1, 0}};     // inverse of a given factor (T^-1 of the natural-gradient step)
static bool listed(const CholIn& in) {
  for (const auto& r : LEGAL)
    if (r[0] == in.want_inverse && r[1] == in.want_transpose && r[2] == in.from_tri && r[3] == in.need_factor && r[4] == in.caller_tbuf) return true;
  return false;
}

// ------------------------------------------------------------------------------------------------ the replay
struct Tile {
  unsigned upd = 0;      // panels whose update it has received
  bool solved = false, parked = false, inplace = false, read_final = false;
};
struct Replay {
  const CholPlan& P;
  int n, T, nb, batch, step = 0, factored = 0;      // T: 64-tiles per side; factored: diagonal blocks done
  std::vector<Tile> tiles;
  std::vector<int> dinv_step;                 // per 128-block: the step that wrote its inverse (-1: none)
  // block rows of the inverse (chol_xrow): per (i, j, 16-column slab) the terms k summed, whether the product with X_ii was applied and when
  struct Slab { unsigned terms = 0; int partial_step = -1, done_step = -1; };
  std::vector<Slab> slabs;
  std::vector<int> xt;                        // per (i, slab): copies of X_ii^T
  // recursive doubling: per 64-tile of X the step that wrote it (-1), per pair (r0 tile) the pending T = L21 X11
  std::vector<int> x64;
  std::map<int64_t, int> pendingT;
  int level;
  Replay(const CholPlan& p) : P(p), n(p.in.n), T(p.in.n / 64), nb(p.nb), batch(p.in.batch), tiles((size_t)T * T), dinv_step((size_t)T, -1),
                              slabs((size_t)T * T * 8), xt((size_t)T * 8, 0), x64((size_t)T * T, -1), level(p.bs) {}
  Tile& tile(int i, int j) {
    REQUIRE(0 <= j && j <= i && i < T, "tile (%d, %d) outside the lower triangle of %d tiles", i, j, T);
    return tiles[(size_t)i * T + j];
  }
  Slab& slab(int i, int j, int cs) { return slabs[((size_t)i * T + j) * 8 + cs]; }
  static unsigned need(int j) { return (1u << (j / 2)) - 1; }      // every panel left of tile column j's block column
  void read_final(int i, int j, const char* who) {
    Tile& t = tile(i, j);
    REQUIRE(t.upd == need(j), "%s (step %d) reads tile (%d, %d) with updates %x, needs %x", who, step, i, j, t.upd, need(j));
    t.read_final = true;
  }
  void update(int i, int j, int p, const char* who) {
    Tile& t = tile(i, j);
    REQUIRE(!t.read_final, "%s (step %d) updates tile (%d, %d) after it was read as final", who, step, i, j);
    REQUIRE(p < j / 2 && !(t.upd >> p & 1), "%s (step %d): update %d of tile (%d, %d), has %x", who, step, p, i, j, t.upd);
    t.upd |= 1u << p;
  }
  // L of 128-block (bi, bk) as an operand: final, and where the reader expects it
  void read_L(int bi, int bk, bool parked, const char* who) {
    for (int a = 2 * bi; a < std::min(T, 2 * bi + 2); ++a)
      for (int b = 2 * bk; b < 2 * bk + 2; ++b) {
        const Tile& t = tile(a, b);
        REQUIRE(t.solved && (parked ? t.parked : t.inplace), "%s (step %d) reads L tile (%d, %d): solved %d parked %d in place %d", who, step, a,
                b, t.solved, t.parked, t.inplace);
      }
  }

  void block(const CholStep& s) {
    const int q = s.q;
    REQUIRE(!P.in.from_tri && q == factored && q < nb, "block %d factored out of order (%d done)", q, factored);
    for (int a = 2 * q; a < std::min(T, 2 * q + 2); ++a)
      for (int b = 2 * q; b <= a; ++b) read_final(a, b, "the diagonal block");
    // side tasks, as k_chol_block deals them: wide-update sub-tiles, then the slabs of xa, then those of xb
    REQUIRE(s.nwide >= 0 && s.xa.nx >= 0 && s.xb.nx >= 0, "negative task counts");
    if (s.nwide) REQUIRE(P.lookahead && q >= 1, "wide update without a parked panel");
    for (int t = 0; t < s.nwide; ++t) {
      int si = 0;
      while ((si + 1) * (si + 2) / 2 <= t) ++si;
      const int sj = t - si * (si + 1) / 2, a = 2 * (q + 1) + si, b = 2 * (q + 1) + sj;
      REQUIRE(a < T, "wide sub-tile %d is row strip %d of %d", t, a, T);
      for (int c = 2 * (q - 1); c < 2 * q; ++c) {
        REQUIRE(tile(a, c).parked && tile(b, c).parked, "wide update of block %d reads an unparked panel tile", q);
      }
      update(a, b, q - 1, "the wide update");
    }
    if (s.xa.nx) xrow(s.xa);
    if (s.xb.nx) xrow(s.xb);
    const int tasks = s.nwide + s.xa.nx + s.xb.nx;
    REQUIRE(s.side <= batch * tasks && s.side <= std::max(32, 248 - batch) && (tasks == 0) == (s.side == 0), "%d side workgroups for %d tasks x %d", s.side, tasks, batch);
    REQUIRE(s.gx == batch + s.side && s.gy == 1, "grid %d x %d", s.gx, s.gy);
    for (int a = 2 * q; a < std::min(T, 2 * q + 2); ++a)
      for (int b = 2 * q; b <= a; ++b) {
        Tile& t = tile(a, b);
        t.solved = true, t.inplace = !(P.items[q].pad & POTRF_PAD_SKIP_WB);
        x64[(size_t)a * T + b] = step;
      }
    dinv_step[q] = step;
    ++factored;
  }

  void xrow(const CholXrowArg& x) {
    const int i = x.i;
    REQUIRE(P.xrows && 0 <= i && i < nb && x.mode >= 0 && x.mode <= 2, "block row %d mode %d", i, x.mode);
    REQUIRE(x.mode == 0 || i == nb - 1, "only the last row is split");
    for (int idx = 0; idx < x.nx; ++idx) {
      const int j = idx >> 3, cs = idx & 7;
      REQUIRE(j <= i, "slab of X(%d, %d)", i, j);
      if (j == i) {      // X_ii^T into the transposed copy
        REQUIRE(P.in.want_transpose && x.mode != 1, "X_ii^T without a transposed output");
        REQUIRE(dinv_step[i] >= 0 && dinv_step[i] < step, "X(%d, %d)^T copied before the block's inverse exists", i, i);
        REQUIRE(++xt[(size_t)i * 8 + cs] == 1, "slab %d of X(%d, %d)^T copied twice", cs, i, i);
        continue;
      }
      Slab& s = slab(i, j, cs);
      REQUIRE(s.done_step < 0, "slab %d of X(%d, %d) written twice", cs, i, j);
      const int k0 = x.mode == 2 ? i - 1 : j, k1 = x.mode == 1 ? i - 1 : i;      // terms [k0, k1)
      REQUIRE(k0 < k1, "no terms for X(%d, %d) in mode %d", i, j, x.mode);
      if (x.mode == 2 && j < i - 1) REQUIRE(s.partial_step >= 0 && s.partial_step < step, "mode 2 of X(%d, %d) without the early terms", i, j);
      if (x.mode == 1) REQUIRE(s.partial_step < 0, "early terms of X(%d, %d) summed twice", i, j);
      for (int k = k0; k < k1; ++k) {
        read_L(i, k, true, "a block row of the inverse");
        if (k == j) REQUIRE(dinv_step[k] >= 0 && dinv_step[k] < step, "X(%d, %d) not final", k, j);
        else
          for (int c = 0; c < 8; ++c) {
            REQUIRE(slab(k, j, c).done_step >= 0 && slab(k, j, c).done_step < step, "X(%d, %d) read before it is final", k, j);
          }
        REQUIRE(!(s.terms >> k & 1), "term %d of X(%d, %d) added twice", k, i, j);
        s.terms |= 1u << k;
      }
      if (x.mode == 1) s.partial_step = step;
      else {
        REQUIRE(dinv_step[i] >= 0 && dinv_step[i] < step, "X(%d, %d) multiplied by X_ii before it exists", i, j);
        REQUIRE(s.terms == ((1u << i) - 1) - ((1u << j) - 1), "X(%d, %d) finished with terms %x", i, j, s.terms);
        s.done_step = step;
      }
    }
  }

  void panel(const CholStep& s) {
    const int p = s.q;
    REQUIRE(P.lookahead && p == factored - 1 && p + 1 < nb, "panel %d after %d blocks", p, factored);
    const int r0 = (p + 1) * 128, nrem = n - r0, nbb = std::min(nrem, 128) / 32;
    std::map<std::pair<int, int>, int> sub;      // 32 x 32 sub-tiles of block column p + 1
    std::vector<int> parked_strip((size_t)nrem / 32, 0);
    for (int idx0 = 0; idx0 < s.gx; ++idx0) {      // k_chol_panel's decode
      int idx = idx0, st, b;
      const int ndiag = nbb * (nbb + 1) / 2;
      if (idx < ndiag) {
        st = 0;
        while ((st + 1) * (st + 2) / 2 <= idx) ++st;
        b = idx - st * (st + 1) / 2;
      } else {
        idx -= ndiag;
        st = nbb + idx / nbb;
        b = idx % nbb;
      }
      const int ra = r0 + 32 * st, rb = r0 + 32 * b;
      REQUIRE(ra + 32 <= n && rb + 32 <= std::min(n, r0 + 128) && rb <= ra, "panel task %d: rows %d, columns %d", idx0, ra, rb);
      const int times = ++sub[std::make_pair(ra / 32, rb / 32)];
      REQUIRE(times == 1, "sub-tile (%d, %d) updated twice", ra / 32, rb / 32);
      for (int c = 2 * p; c < 2 * p + 2; ++c) read_final(ra / 64, c, "the panel solve"), read_final(rb / 64, c, "the panel solve");
      if (b == 0) ++parked_strip[(size_t)st];
    }
    REQUIRE(dinv_step[p] >= 0 && dinv_step[p] < step, "panel %d before its block's inverse", p);
    for (size_t st = 0; st < parked_strip.size(); ++st) REQUIRE(parked_strip[st] == 1, "strip %zu of panel %d parked %d times", st, p, parked_strip[st]);
    for (int a = 2 * (p + 1); a < T; ++a) {
      for (int c = 2 * p; c < 2 * p + 2; ++c) tile(a, c).solved = tile(a, c).parked = true;
      for (int b = 2 * (p + 1); b <= std::min(a, 2 * (p + 1) + 1); ++b) {
        int got = 0;
        for (int u = 0; u < 2; ++u)
          for (int v = 0; v < 2; ++v) got += (int)sub.count(std::make_pair(2 * a + u, 2 * b + v));
        REQUIRE(got == (a == b ? 3 : 4), "tile (%d, %d) got %d sub-tile updates of panel %d", a, b, got, p);
        update(a, b, p, "the panel launch");
      }
    }
    REQUIRE(s.gy == batch && s.gx >= 1, "grid %d x %d", s.gx, s.gy);
  }

  static bool same(const CholRef& a, int buf, int64_t off) { return a.buf == buf && a.off == off; }
  void gemm(const CholStep& s) {
    REQUIRE(s.count >= 1 && s.first >= 0 && s.first + s.count <= (int)P.gemms.size() && s.gy == 1, "problems [%d, + %d)", s.first, s.count);
    int tiles = 0;
    const int64_t N = n;
    for (int e = s.first; e < s.first + s.count; ++e) {
      const CholGemm& g = P.gemms[(size_t)e];
      tiles += ((g.m + 63) / 64) * ((g.n + 63) / 64) * batch;
      const int cr = (int)(g.C.off / N), cc = (int)(g.C.off % N);
      REQUIRE(cr % 64 == 0 && cc % 64 == 0 && g.m % 64 == 0 && g.n % 64 == 0 && g.k % 64 == 0 && g.m > 0 && g.n > 0 && g.k > 0, "problem %d is not whole tiles", e);
      if (g.C.buf == CB_W && cc > cr) {      // plain form: the panel solve, transposed into the mirror blocks
        const int p = cr / 128, rem = n - (p + 1) * 128;
        REQUIRE(!P.lookahead && !P.in.from_tri && s.count == 1 && p == factored - 1 && cr == p * 128 && cc == (p + 1) * 128 && rem > 0, "panel solve %d", p);
        REQUIRE(g.m == 128 && g.n == rem && g.k == 128 && !g.transA && g.transB && g.alpha == 1.0 && g.beta == 0.0 && !g.lower_only && g.tri == 2, "panel solve %d: shape", p);
        REQUIRE(g.A.buf == P.items[p].inv.buf && g.A.off == P.items[p].inv.off && same(g.B, CB_W, (int64_t)cc * N + cr), "panel solve %d: operands", p);
        for (int a = 2 * (p + 1); a < T; ++a)
          for (int c = 2 * p; c < 2 * p + 2; ++c) {
            read_final(a, c, "the panel solve");
            tile(a, c).solved = tile(a, c).parked = true;
          }
      } else if (g.C.buf == CB_W) {          // plain form: the trailing update
        const int p = cr / 128 - 1, rem = n - cr;
        REQUIRE(!P.lookahead && s.count == 1 && cr == cc && p == factored - 1 && p >= 0, "trailing update %d", p);
        const int64_t mirror = (int64_t)p * 128 * N + (p + 1) * 128;
        REQUIRE(same(g.A, CB_W, mirror) && same(g.B, CB_W, mirror) && g.transA && !g.transB && g.m == rem && g.n == rem && g.k == 128 && g.alpha == -1.0 &&
                    g.beta == 1.0 && g.lower_only == 1 && g.tri == 0, "trailing update %d: operands", p);
        for (int a = 2 * (p + 1); a < T; ++a) {
          REQUIRE(tile(a, 2 * p).parked && tile(a, 2 * p + 1).parked, "trailing update %d reads an unparked panel", p);
          for (int b = 2 * (p + 1); b <= a; ++b) update(a, b, p, "the trailing update");
        }
      } else if (g.C.buf == CB_S) {          // recursive doubling: T = L21 X11
        const int sblk = g.n, rows = g.m;
        REQUIRE(P.in.want_inverse && !P.xrows && sblk == level && cc + sblk == cr && cc % (2 * sblk) == 0 && rows == std::min(sblk, n - cr) && g.k == sblk,
                "T product at (%d, %d): block %d, level %d", cr, cc, sblk, level);
        REQUIRE(same(g.A, CB_W, g.C.off) && same(g.B, CB_LINV, (int64_t)cc * N + cc) && !g.transA && !g.transB && g.alpha == 1.0 && g.beta == 0.0 && g.tri == 1 && !g.lower_only, "T product: operands");
        for (int a = cr / 64; a < (cr + rows) / 64; ++a)
          for (int b = cc / 64; b < cr / 64; ++b) {
            REQUIRE(tile(a, b).solved && tile(a, b).inplace, "T product reads L tile (%d, %d) that is not in place", a, b);
          }
        require_x_block(cc, sblk, "X11");
        REQUIRE(pendingT.emplace(g.C.off, step).second, "pair at row %d covered twice", cr);
      } else {                               // X21 = -X22 T
        const int sblk = g.n, rows = g.m;
        REQUIRE(g.C.buf == CB_LINV && sblk == level && g.k == rows && cc + sblk == cr, "X21 product at (%d, %d)", cr, cc);
        REQUIRE(same(g.A, CB_LINV, (int64_t)cr * N + cr) && same(g.B, CB_S, g.C.off) && !g.transA && !g.transB && g.alpha == -1.0 && g.beta == 0.0 && g.tri == 2 && !g.lower_only, "X21 product: operands");
        const auto it = pendingT.find(g.C.off);
        REQUIRE(it != pendingT.end() && it->second < step, "X21 at row %d without its T", cr);
        pendingT.erase(it);
        require_x_block(cr, rows, "X22");
        for (int a = cr / 64; a < (cr + rows) / 64; ++a)
          for (int b = cc / 64; b < cr / 64; ++b) {
            REQUIRE(x64[(size_t)a * T + b] < 0, "X tile (%d, %d) written twice", a, b);
            x64[(size_t)a * T + b] = step;
          }
      }
    }
    REQUIRE(s.gx == tiles && tiles >= 1, "grid %d, %d tiles", s.gx, tiles);
    // the end of a level: every pair covered — all diagonal blocks of twice the size are whole
    const CholGemm& last = P.gemms[(size_t)s.first];
    if (last.C.buf == CB_LINV) {
      REQUIRE(pendingT.empty(), "a T product of level %d has no X21 product", level);
      level *= 2;
      for (int c0 = 0; c0 < n; c0 += level) require_x_block(c0, std::min(level, n - c0), "a doubled block", step + 1);
    }
  }
  void require_x_block(int c0, int size, const char* who, int before = -1) {      // final before step `before` (default: this one)
    if (before < 0) before = step;
    for (int a = c0 / 64; a < (c0 + size) / 64; ++a)
      for (int b = c0 / 64; b <= a; ++b) REQUIRE(x64[(size_t)a * T + b] >= 0 && x64[(size_t)a * T + b] < before, "%s: X tile (%d, %d) is not final before step %d", who, a, b, before);
  }

  void run() {
    if (P.in.from_tri)
      for (int a = 0; a < T; ++a)
        for (int b = 0; b <= a; ++b) tile(a, b).solved = tile(a, b).inplace = true, tile(a, b).upd = need(b);
    bool mirrored = false, transposed = false;
    for (const CholStep& s : P.steps) {
      REQUIRE(s.gx >= 1 && s.gy >= 1 && !transposed, "step %d (%s)", step, show(s).c_str());
      switch (s.kind) {
        case CS_BLOCK: block(s); break;
        case CS_PANEL: panel(s); break;
        case CS_GEMM: gemm(s); break;
        case CS_XROW_LAST:
          REQUIRE(factored == nb && s.q == nb - 1 && s.xa.i == nb - 1 && s.xa.mode == 2 && s.xa.nx >= 1, "last row launch");
          REQUIRE(s.gx <= 2048 && s.gx <= batch * s.xa.nx && s.gy == 1, "grid %d", s.gx);
          xrow(s.xa);
          break;
        case CS_TRTRI_DIAG64:
          REQUIRE(P.in.from_tri && step == 0 && s.gx == nb * batch && s.gy == 1 && nb == T, "diagonal inverses");
          for (int a = 0; a < T; ++a) x64[(size_t)a * T + a] = step;
          break;
        case CS_MIRROR:
          REQUIRE(!P.in.from_tri && factored == nb && !mirrored && s.gx <= 1024 && s.gy == batch, "mirror");
          for (int a = 0; a < T; ++a)
            for (int b = 0; b <= a; ++b)
              if (tile(a, b).parked) tile(a, b).parked = false, tile(a, b).inplace = true;
          mirrored = true;
          break;
        case CS_TRANSPOSE:
          REQUIRE(P.in.want_transpose && !P.xrows && s.gx == 256 && s.gy == batch, "transpose");
          require_x_block(0, n, "the transpose");
          transposed = true;
          break;
        default: REQUIRE(false, "unknown step kind %d", s.kind);
      }
      ++step;
    }
    // the end: L everywhere (and in place for a caller that reads it), X whole and written once, its transpose whole
    if (!P.in.from_tri) REQUIRE(factored == nb, "%d of %d blocks factored", factored, nb);
    for (int a = 0; a < T; ++a)
      for (int b = 0; b <= a; ++b) {
        REQUIRE(tile(a, b).solved && tile(a, b).upd == need(b), "tile (%d, %d) is not final at the end", a, b);
        if (P.in.need_factor) REQUIRE(tile(a, b).inplace && !tile(a, b).parked, "the caller reads L but tile (%d, %d) is not in place", a, b);
      }
    if (P.in.want_inverse && P.xrows) {
      for (int i = 0; i < nb; ++i) {
        REQUIRE(dinv_step[i] >= 0, "X(%d, %d) missing", i, i);
        for (int cs = 0; cs < 8; ++cs) {
          for (int j = 0; j < i; ++j) REQUIRE(slab(i, j, cs).done_step >= 0, "slab %d of X(%d, %d) missing", cs, i, j);
          REQUIRE(xt[(size_t)i * 8 + cs] == (P.in.want_transpose ? 1 : 0), "slab %d of X(%d, %d)^T: %d copies", cs, i, i, xt[(size_t)i * 8 + cs]);
        }
      }
    } else if (P.in.want_inverse) {
      require_x_block(0, n, "the end");
      REQUIRE(level >= n && transposed == P.in.want_transpose, "doubling stopped at %d", level);
    }
  }
};

// ------------------------------------------------------------------------------------------------ memory, items
struct Rect { int buf; int64_t off; int rows, cols; };
static bool overlap(const Rect& a, const Rect& b, int n) {
  if (a.buf != b.buf) return false;
  const int64_t ar = a.off / n, ac = a.off % n, br = b.off / n, bc = b.off % n;
  return ar < br + b.rows && br < ar + a.rows && ac < bc + b.cols && bc < ac + a.cols;
}
static void check_memory(const CholPlan& P) {
  const CholIn& in = P.in;
  const int n = in.n;
  const int64_t NN = (int64_t)n * n;
  int64_t size[CB_COUNT], end[CB_COUNT] = {0, 0, 0, 0};      // doubles the buffer holds; the furthest double of matrix 0 a step touches
  size[CB_W] = in.batch * NN;
  size[CB_LINV] = in.want_inverse ? in.batch * NN : 0;
  size[CB_TBUF] = in.caller_tbuf ? (int64_t)in.batch * 128 * n : (int64_t)(P.tbuf_bytes / 8);
  size[CB_S] = in.want_transpose ? in.batch * NN : (int64_t)(P.s_bytes / 8);
  auto touch = [&](const Rect& r, const char* who) {
    REQUIRE(r.buf >= 0 && r.buf < CB_COUNT && r.off >= 0 && r.rows >= 1 && r.cols >= 1 && r.off % n + r.cols <= n, "%s: buffer %d offset %lld, %d x %d", who, r.buf, (long long)r.off, r.rows, r.cols);
    const int64_t e = r.off + (int64_t)(r.rows - 1) * n + r.cols;
    REQUIRE(e <= P.stride[r.buf] && (int64_t)in.batch * P.stride[r.buf] <= size[r.buf], "%s: ends at %lld of a matrix of %lld, buffer %d holds %lld", who, (long long)e, (long long)P.stride[r.buf], r.buf, (long long)size[r.buf]);
    end[r.buf] = std::max(end[r.buf], e);
  };
  for (const CholItem& it : P.items) {
    touch(Rect{CB_W, it.w_off, it.bn, it.bn}, "a diagonal block");
    touch(Rect{it.inv.buf, it.inv.off, it.bn, it.bn}, "a diagonal block's inverse");
  }
  for (const CholStep& s : P.steps) {
    if (s.kind != CS_GEMM) continue;
    std::vector<Rect> out;
    for (int e = s.first; e < s.first + s.count; ++e) {
      const CholGemm& g = P.gemms[(size_t)e];
      const Rect A{g.A.buf, g.A.off, g.transA ? g.k : g.m, g.transA ? g.m : g.k}, B{g.B.buf, g.B.off, g.transB ? g.n : g.k, g.transB ? g.k : g.n},
          C{g.C.buf, g.C.off, g.m, g.n};
      touch(A, "A"), touch(B, "B"), touch(C, "C");
      for (const Rect& o : out) REQUIRE(!overlap(o, C, n), "two problems of one launch write overlapping regions");
      out.push_back(C);
      // (GEMM_SMALL_K of linalg.hip: a launch short in k may take the LDS-free kernel, whose waves read A and B while others store C)
      if (g.k <= 256 && g.k % 16 == 0) REQUIRE(!overlap(A, C, n) && !overlap(B, C, n), "problem %d updates an operand in place", e);
    }
  }
  // what the plan owns is what the steps touch: whole rows of n doubles per matrix, nothing when nothing is touched
  for (int b : {CB_TBUF, CB_S}) {
    const int64_t owned = b == CB_TBUF ? (int64_t)P.tbuf_bytes : (int64_t)P.s_bytes;
    const bool lent = b == CB_TBUF ? in.caller_tbuf : in.want_transpose;
    if (lent) REQUIRE(owned == 0, "the plan allocates buffer %d although the caller lends it", b);
    else REQUIRE(owned == (end[b] + n - 1) / n * n * 8 * in.batch, "buffer %d: %lld bytes owned, the steps reach double %lld of a matrix", b, (long long)owned, (long long)end[b]);
  }
  REQUIRE(P.items_bytes >= (in.from_tri ? (size_t)P.nb * in.batch * CHOL_ITEM_BYTES : 0) && P.desc_bytes >= P.items_bytes + P.gemms.size() * CHOL_GEMM_BYTES && P.items_bytes % 256 == 0,
          "descriptor block of %zu bytes", P.desc_bytes);
}

static void check_items(const CholPlan& P) {
  const CholIn& in = P.in;
  REQUIRE(P.bs == (in.from_tri ? 64 : 128) && P.nb == (in.n + P.bs - 1) / P.bs && (int)P.items.size() == P.nb, "%d blocks of %d", P.nb, P.bs);
  int sum = 0, row = 0;
  for (int p = 0; p < P.nb; ++p) {
    const CholItem& it = P.items[(size_t)p];
    REQUIRE(it.info_offset == row && it.w_off == (int64_t)row * in.n + row && (it.bn == 64 || it.bn == P.bs) && row + it.bn <= in.n, "block %d starts at row %d", p, row);
    REQUIRE(((it.pad & POTRF_PAD_ACCUM) != 0) == (p > 0), "block %d: scal is %s", p, p ? "set" : "accumulated");
    REQUIRE(((it.pad & POTRF_PAD_SKIP_WB) != 0) == (P.xrows && !in.need_factor) && !(it.pad & ~(POTRF_PAD_ACCUM | POTRF_PAD_SKIP_WB)) && it.pad != POTRF_PAD_TIMING, "block %d: pad %d", p, it.pad);
    REQUIRE(it.nreal >= 0 && it.nreal <= it.bn && it.nreal == std::max(0, std::min(it.bn, in.nreal - row)), "block %d: real order %d", p, it.nreal);
    REQUIRE(in.want_inverse ? (it.inv.buf == CB_LINV && it.inv.off == it.w_off) : it.inv.buf == CB_TBUF, "block %d: where its inverse goes", p);
    sum += it.nreal, row += it.bn;
  }
  REQUIRE(sum == in.nreal && row == in.n, "the blocks hold %d real rows of %d", sum, in.nreal);
  REQUIRE(P.lookahead == (!in.from_tri && in.lookahead_allowed && P.nb >= 2 && P.nb <= 16) && P.xrows == (P.lookahead && in.want_inverse), "look-ahead %d, block rows %d", P.lookahead, P.xrows);
  for (const CholStep& s : P.steps) REQUIRE(P.lookahead || (s.kind != CS_PANEL && s.kind != CS_XROW_LAST && (s.kind != CS_BLOCK || s.side == 0)), "a look-ahead launch in the plain sequence");
}

static void check_plan(const CholIn& in) {
  g_what = describe(in);
  const CholPlan P = chol_plan(in);
  REQUIRE(P.ok == listed(in) && chol_in_legal(in) == P.ok, "the planner %s a call that is %s", P.ok ? "accepts" : "refuses", listed(in) ? "listed" : "not listed");
  ++g_checks;
  if (!P.ok) return;
  Replay(P).run();      // coverage of the factorisation, the inverse, the grids of the steps
  g_checks += 3;
  check_memory(P);
  ++g_checks;
  check_items(P);
  ++g_checks;
}

// ------------------------------------------------------------------------------------------------ the route
static void check_route() {
  g_what = "route";
  for (int n = 1; n <= 2304; ++n) {
    // dsdgp_potrf as it was
    const int np = n > 176 ? (n + 63) / 64 * 64 : (n + 15) / 16 * 16;
    const CholRoute r = chol_route(n, CHOL_BLOCKED_MIN, true);
    REQUIRE(r.np == np && (r.kind == CHOL_BLOCKED) == (np >= 192 && np % 64 == 0) && (r.kind == CHOL_ONE_WG_LDS) == (np <= 128), "dsdgp_potrf at n = %d: order %d kind %d", n, r.np, r.kind);
    for (int thr : {128, 192}) {
      if (n % 16 == 0) {      // a layer's Mp (model.hip) and what potrf_launch did with the others
        const CholRoute m = chol_route(n, thr, false);
        REQUIRE(m.np == n && (m.kind == CHOL_BLOCKED) == (n >= thr && n % 64 == 0) && (m.kind == CHOL_BLOCKED || (m.kind == CHOL_ONE_WG_LDS) == (n <= 128)), "Mp = %d, threshold %d: kind %d", n, thr, m.kind);
      }
    }
    const int Mp = pad_M(n);      // model_layout.hpp's uniform batch
    REQUIRE((chol_route(Mp, CHOL_BLOCKED_MIN, false).kind == CHOL_BLOCKED) == (Mp >= 192 && Mp % 64 == 0), "uniform batch at M = %d", n);
    if (n % 16 == 0) {      // potrf_launch as it was
      const size_t base = (16 * 17 + 8 + (size_t)(n / 16) * 16 * 17) * 8;
      const PotrfLds l = potrf_lds(n);
      REQUIRE(l.nb_max == n / 16 && l.in_lds == (n <= 128) && l.bytes == (n <= 128 ? base + (size_t)n * (n + 4) * 8 : base), "potrf_lds(%d)", n);
    }
    ++g_checks;
  }
  REQUIRE(CHOL_BLOCKED_MIN == 192, "the threshold in use");
  // more than 16 blocks: the plain sequence, the one DSDGP_CHOL_LOOKAHEAD=0 selects below that
  auto kinds = [](int n, bool allowed) {
    const CholPlan P = chol_plan(CholIn{n, n - 20, 1, true, true, false, false, false, allowed});
    REQUIRE(P.ok && !P.lookahead && !P.xrows, "n = %d takes the look-ahead form", n);
    std::string k, out;
    for (const CholStep& s : P.steps) k += "BPGXTMR"[s.kind];
    // the per-panel group and the doubling levels, however often repeated
    for (size_t i = 0; i < k.size();) {
      const std::string grp = k.compare(i, 3, "BGG") == 0 ? "BGG" : (k.compare(i, 2, "GG") == 0 ? "GG" : k.substr(i, 1));
      while (k.compare(i, grp.size(), grp) == 0) i += grp.size();
      out += "(" + grp + ")";
    }
    return out;
  };
  for (int n = 2112; n <= 2304; n += 64) REQUIRE(kinds(n, true) == kinds(1152, false), "n = %d: %s, n = 1152 without look-ahead: %s", n, kinds(n, true).c_str(), kinds(1152, false).c_str());
  REQUIRE(kinds(1152, false) == "(BGG)(B)(M)(GG)(R)", "the plain sequence is %s", kinds(1152, false).c_str());
  ++g_checks;
}

// ------------------------------------------------------------------------------------------------ the pinned table
struct Pinned { CholIn in; std::vector<const char*> steps; };
static const char* B0 = "B q=0 g=1 w=0 xa=-1/0/0 xb=-1/0/0 s=0";
static void check_pinned() {
  const std::vector<Pinned> table = {
      // Ku of a model (Linv + LinvT, white = False), look-ahead
      {{192, 180, 1, true, true, false, false, false, true}, {B0, "P p=0 g=3x1", "B q=1 g=9 w=0 xa=0/8/0 xb=1/0/1 s=8", "X i=1 nx=16 m=2 g=16"}},
      {{320, 300, 1, true, true, false, false, false, true},
       {B0, "P p=0 g=18x1", "B q=1 g=10 w=1 xa=0/8/0 xb=0/0/0 s=9", "P p=1 g=3x1", "B q=2 g=25 w=0 xa=1/16/0 xb=2/8/1 s=24", "X i=2 nx=24 m=2 g=24"}},
      {{1024, 1024, 3, true, true, false, false, false, true},
       {"B q=0 g=3 w=0 xa=-1/0/0 xb=-1/0/0 s=0", "P p=0 g=106x3", "B q=1 g=248 w=78 xa=0/8/0 xb=0/0/0 s=245", "P p=1 g=90x3",
        "B q=2 g=216 w=55 xa=1/16/0 xb=1/0/0 s=213", "P p=2 g=74x3", "B q=3 g=183 w=36 xa=2/24/0 xb=2/0/0 s=180", "P p=3 g=58x3",
        "B q=4 g=162 w=21 xa=3/32/0 xb=3/0/0 s=159", "P p=4 g=42x3", "B q=5 g=153 w=10 xa=4/40/0 xb=4/0/0 s=150", "P p=5 g=26x3",
        "B q=6 g=156 w=3 xa=5/48/0 xb=5/0/0 s=153", "P p=6 g=10x3", "B q=7 g=248 w=0 xa=6/56/0 xb=7/48/1 s=245", "X i=7 nx=64 m=2 g=192"}},
      // the same with DSDGP_CHOL_LOOKAHEAD=0
      {{320, 300, 1, true, true, false, false, false, false},
       {B0, "G f=0 c=1 big=0 g=6", "G f=1 c=1 big=0 g=9", "B q=1 g=1 w=0 xa=0/0/0 xb=0/0/0 s=0", "G f=2 c=1 big=0 g=2", "G f=3 c=1 big=0 g=1",
        "B q=2 g=1 w=0 xa=1/0/0 xb=1/0/0 s=0", "M g=400x1", "G f=4 c=1 big=0 g=4", "G f=5 c=1 big=0 g=4", "G f=6 c=1 big=0 g=4", "G f=7 c=1 big=0 g=4",
        "Tr g=256x1"}},
      // T^-1 of the natural-gradient step
      {{640, 600, 2, true, false, true, true, false, true},
       {"T g=20", "G f=0 c=5 big=0 g=10", "G f=5 c=5 big=0 g=10", "G f=10 c=2 big=0 g=16", "G f=12 c=2 big=0 g=16", "G f=14 c=1 big=0 g=32",
        "G f=15 c=1 big=0 g=32", "G f=16 c=1 big=1 g=32", "G f=17 c=1 big=1 g=32"}},
      // dsdgp_potrf
      {{256, 200, 1, false, false, false, true, false, true}, {B0, "P p=0 g=10x1", "B q=1 g=1 w=0 xa=0/0/0 xb=0/0/0 s=0", "M g=256x1"}}};
  for (const Pinned& t : table) {
    g_what = "pinned: " + describe(t.in);
    const CholPlan P = chol_plan(t.in);
    REQUIRE(P.ok && P.steps.size() == t.steps.size(), "%zu steps, %zu pinned", P.steps.size(), t.steps.size());
    for (size_t i = 0; i < t.steps.size(); ++i) REQUIRE(show(P.steps[i]) == t.steps[i], "step %zu is \"%s\", pinned \"%s\"", i, show(P.steps[i]).c_str(), t.steps[i]);
    ++g_checks;
  }
}

int main() {
  check_pinned();
  check_route();
  long plans = 0, refused = 0;
  for (int n = 128; n <= 2304; n += 64)
    for (int d : {0, 1, 63, 64, 127})
      for (int batch : {1, 2, 5, 17})
        for (int f = 0; f < 64; ++f) {
          const CholIn in{n, n - d, batch, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0, (f & 16) != 0, (f & 32) != 0};
          if (in.nreal < 1) continue;
          // (the refused combinations do not depend on the sizes: once per n)
          if (!listed(in) && (d || batch > 1)) continue;
          check_plan(in);
          ++(listed(in) ? plans : refused);
        }
  for (const CholIn& bad : {CholIn{64, 64, 1, false, false, false, true, false, true}, CholIn{200, 200, 1, false, false, false, true, false, true},
                            CholIn{256, 256, 0, false, false, false, true, false, true}, CholIn{256, 0, 1, false, false, false, true, false, true},
                            CholIn{256, 257, 1, false, false, false, true, false, true}}) {
    g_what = describe(bad);
    REQUIRE(!chol_plan(bad).ok, "accepted");
    ++g_checks, ++refused;
  }
  printf("chol_plan_check: %ld plans replayed, %ld calls refused, %ld checks, every invariant holds\n", plans, refused, g_checks);
  return 0;
}
