// Host plan of the Cholesky factorisations: which kernel family takes a matrix of a given order (chol_route), the one-workgroup
// kernel's LDS (potrf_lds), and the whole launch sequence of the multi-workgroup blocked Cholesky + triangular inverse (chol_plan) as a
// list of steps over (buffer, offset) operands.  linalg.hip binds the operands to pointers and walks the steps; nothing there decides.
// No HIP and no pointer: tests/host/chol_plan_check.cpp compiles it alone and replays every plan against the algorithm.
#pragma once
#include "plan_types.hpp"
#include <vector>

// PotrfItem::pad (linalg.hpp)
enum { POTRF_PAD_TIMING = 7,      // the value: phase clocks of the one-workgroup kernel into scal[2..] (debug aid)
       POTRF_PAD_SKIP_WB = 8,     // bit: the factor is not written back (nobody reads it)
       POTRF_PAD_ACCUM = 16 };    // bit: log det / info are added to what scal holds (the later blocks of the blocked sequence)

// ---- the route ----
// Padded inducing count / matrix order from which the multi-workgroup blocked sequence replaces the one-workgroup kernel.  Measured,
// factor + inverse of one matrix: at this order 180 -> 77 us, at 256 371 -> 101, at 448 1990 -> 181.
#define CHOL_BLOCKED_MIN 192
#define CHOL_ONE_WG_LDS_MAX 128      // largest order whose working matrix the one-workgroup kernel keeps in LDS
enum CholRouteKind { CHOL_ONE_WG_LDS, CHOL_ONE_WG_GLOBAL, CHOL_BLOCKED };
struct CholRoute { int np; CholRouteKind kind; };
// n: the order.  may_pad: the caller copies the matrix into a buffer of the padded order (dsdgp_potrf) and the route picks the padding;
// otherwise n is a padded order fixed elsewhere (a model's Mp: a multiple of 16) and the blocked sequence takes it only as a multiple of 64.
static inline CholRoute chol_route(int n, int blocked_min, bool may_pad) {
  int np = (int)round_up(n, 16);
  if (np >= blocked_min) {
    if (may_pad) np = (int)round_up(n, 64);
    if (np % 64 == 0) return CholRoute{np, CHOL_BLOCKED};
  }
  return CholRoute{np, np <= CHOL_ONE_WG_LDS_MAX ? CHOL_ONE_WG_LDS : CHOL_ONE_WG_GLOBAL};
}

// k_potrf_trtri: dynamic LDS of a launch whose largest item has order n_max — the diagonal-block inverses and scratch, and up to
// CHOL_ONE_WG_LDS_MAX the n x (n + 4) working matrix
struct PotrfLds { bool in_lds; int nb_max; size_t bytes; };
static inline PotrfLds potrf_lds(int n_max) {
  PotrfLds r{n_max <= CHOL_ONE_WG_LDS_MAX, n_max / 16, 0};
  r.bytes = (16 * 17 + 8 + (size_t)r.nb_max * 16 * 17) * sizeof(double);
  if (r.in_lds) r.bytes += (size_t)n_max * (n_max + 4) * sizeof(double);
  return r;
}

// ---- the blocked sequence ----
#define BCB 128               // diagonal block of the blocked factorisation (64 for the inverse of a given factor)
#define CHOL_ITEM_BYTES 56    // sizeof(PotrfItem), sizeof(GemmProblem): linalg.hip asserts them
#define CHOL_GEMM_BYTES 152

// The call as plain values.  Legal: want_transpose, from_tri and !need_factor need want_inverse; from_tri (the input is a lower-triangular
// factor, only its inverse is formed) excludes want_transpose and keeps need_factor; caller_tbuf (the caller lends the scratch that holds
// the diagonal blocks' inverses) only without want_inverse, where they live in Linv.  lookahead_allowed is free.
struct CholIn {
  int n, nreal, batch;      // n: padded order, a multiple of 64 from 128 on; rows / columns from nreal on carry an identity pad
  bool want_inverse, want_transpose, from_tri, need_factor, caller_tbuf, lookahead_allowed;
};
static inline bool chol_in_legal(const CholIn& in) {
  if (in.n < 128 || in.n % 64 != 0 || in.batch < 1 || in.nreal < 1 || in.nreal > in.n) return false;
  if (!in.want_inverse && (in.want_transpose || in.from_tri || !in.need_factor)) return false;
  if (in.from_tri && (in.want_transpose || !in.need_factor)) return false;
  return !(in.caller_tbuf && in.want_inverse);
}

// W, Linv: the caller's (batch matrices of order n, n * n doubles apart); Tbuf: bs x n per matrix; S: n x n per matrix, the scratch of the
// recursive doubling — the caller's LinvT when it wants the transpose (the final transpose overwrites it), else the plan's
enum CholBuf { CB_W, CB_LINV, CB_TBUF, CB_S, CB_COUNT };
struct CholRef { int buf; int64_t off; };      // off in doubles, matrix 0; matrix b: + b * stride[buf]
struct CholItem {      // one diagonal block (matrix 0)
  int64_t w_off;       // into W
  CholRef inv;         // where its inverse goes: Linv's diagonal, or Tbuf without a requested inverse (the panel solve needs it)
  int bn, nreal, pad, info_offset;
};
struct CholGemm {      // C = alpha op(A) op(B) + beta C, every leading dimension n, batch strides by buffer
  CholRef A, B, C;
  int m, n, k, transA, transB;
  double alpha, beta;
  int lower_only, tri;
};
enum CholStepKind { CS_BLOCK, CS_PANEL, CS_GEMM, CS_XROW_LAST, CS_TRTRI_DIAG64, CS_MIRROR, CS_TRANSPOSE };
struct CholXrowArg { int i, nx, mode; };
struct CholStep {
  int kind, gx, gy;            // one launch and its grid (GEMM: gx = the 64 x 64 tiles; gemm_plan may take the 128 x 128 kernel for allow_big 1)
  int q;                       // BLOCK: the diagonal block; PANEL: the panel; XROW_LAST: the row
  int nwide, side;             // BLOCK: wide-update sub-tiles per matrix; side workgroups of the launch (gx = batch + side)
  CholXrowArg xa, xb;          // BLOCK: the two block rows of the inverse its side workgroups form; XROW_LAST: xa
  int first, count, allow_big; // GEMM: problems [first, first + count) planned together
};
struct CholPlan {
  bool ok;      // false: an illegal CholIn, nothing else is set
  CholIn in;
  int nb, bs;
  bool lookahead;      // k_chol_panel between the diagonal blocks, the wide update inside the factor launches
  bool xrows;          // ... and the block rows of the inverse (chol_xrow) instead of the recursive doubling
  int64_t stride[CB_COUNT];
  size_t tbuf_bytes, s_bytes, desc_bytes;      // what the plan owns: Tbuf (zeroed), S, then the device items and GEMM problems
  size_t items_bytes;                          // the items' share of desc_bytes (k_trtri_diag64 reads them; k_chol_block gets its item as an argument)
  std::vector<CholItem> items;
  std::vector<CholGemm> gemms;
  std::vector<CholStep> steps;
};

static inline int chol_gemm_tiles(const CholGemm& g, int batch) { return ceil_div(g.m, 64) * ceil_div(g.n, 64) * batch; }

static inline CholPlan chol_plan(const CholIn& in) {
  CholPlan P{};
  P.ok = chol_in_legal(in);
  if (!P.ok) return P;
  P.in = in;
  const int n = in.n, batch = in.batch;
  const int bs = P.bs = in.from_tri ? 64 : BCB;
  const int nb = P.nb = ceil_div(n, bs);
  // the wide-update workgroups of the look-ahead form each hold a whole CU (the factor launch's LDS): beyond 16 blocks the plain sequence
  P.lookahead = !in.from_tri && in.lookahead_allowed && nb >= 2 && nb <= 16;
  P.xrows = in.want_inverse && P.lookahead;
  const int64_t N = n;
  P.stride[CB_W] = P.stride[CB_LINV] = P.stride[CB_S] = N * N;
  P.stride[CB_TBUF] = (int64_t)bs * N;
  for (int p = 0; p < nb; ++p) {
    const int bn = std::min(bs, n - p * bs);      // 64 at a ragged end
    const int64_t off = (int64_t)p * bs * N + p * bs;
    // block 0 SETS log det / info, the later blocks accumulate: no memset of `scal` in front of the sequence.  With the inverse formed from
    // the parked panels and nobody reading L, the block's own write-back goes too
    const int pad = (p ? POTRF_PAD_ACCUM : 0) | (P.xrows && !in.need_factor ? POTRF_PAD_SKIP_WB : 0);
    P.items.push_back(CholItem{off, in.want_inverse ? CholRef{CB_LINV, off} : CholRef{CB_TBUF, (int64_t)p * bs}, bn,
                               std::max(0, std::min(bn, in.nreal - p * bs)), pad, p * bs});
  }
  auto gemm_step = [&](int count, int allow_big) {
    CholStep s{};
    s.kind = CS_GEMM, s.first = (int)P.gemms.size() - count, s.count = count, s.allow_big = allow_big, s.gy = 1;
    for (int i = 0; i < count; ++i) s.gx += chol_gemm_tiles(P.gemms[s.first + i], batch);
    P.steps.push_back(s);
  };
  if (!in.from_tri) {
    for (int p = 0; p < nb; ++p) {
      CholStep s{};
      s.kind = CS_BLOCK, s.q = p, s.gy = 1;
      s.xa = s.xb = CholXrowArg{p - 1, 0, 0};
      if (P.lookahead && p >= 1) {
        const int ns64 = std::max(0, n - (p + 1) * BCB) / 64;      // 64-row strips from block p + 1 on
        s.nwide = ns64 * (ns64 + 1) / 2;
      }
      if (P.xrows && p >= 1) s.xa.nx = 8 * (p - 1 + (in.want_transpose ? 1 : 0));
      if (P.xrows && p == nb - 1) s.xb = CholXrowArg{p, 8 * (p - 1), 1};      // the early terms of the last row
      s.side = std::min(batch * (s.nwide + s.xa.nx + s.xb.nx), std::max(32, 248 - batch));      // (a CU each: one round of them)
      s.gx = batch + s.side;
      P.steps.push_back(s);
      if (p + 1 == nb) break;
      const int rem = n - (p + 1) * BCB;
      if (P.lookahead) {
        const int nbb = std::min(rem, BCB) / 32, ns = rem / 32;      // 32 x 32 sub-tiles of block column p + 1, its diagonal block's lower ones
        CholStep t{};
        t.kind = CS_PANEL, t.q = p, t.gx = nbb * (nbb + 1) / 2 + (ns - nbb) * nbb, t.gy = batch;
        P.steps.push_back(t);
      } else {
        // the panel, TRANSPOSED, into the mirror blocks above the diagonal (unused by the factorisation):  L_ip^T = L_pp^-1 A_ip^T.
        // Out of place, so the LDS-free 64 x 64 kernel can take it (16 us; in place only a kernel whose workgroup owns all 128 columns
        // of its rows is safe — the 128 x 128 kernel at 8 barrier-separated k-steps: 26 us).  k_mirror_panels moves the panels
        // back below the diagonal at the end.
        const CholRef panel{CB_W, (int64_t)(p + 1) * BCB * N + p * BCB}, mirror{CB_W, (int64_t)p * BCB * N + (p + 1) * BCB};
        P.gemms.push_back(CholGemm{P.items[p].inv, panel, mirror, BCB, rem, BCB, 0, 1, 1.0, 0.0, 0, 2});      // L_pp^-1 lower-triangular
        gemm_step(1, 0);
        // A_ij -= L_ip L_jp^T  (lower tiles only), both operands read from the transposed panel
        P.gemms.push_back(CholGemm{mirror, mirror, CholRef{CB_W, (int64_t)(p + 1) * BCB * (N + 1)}, rem, rem, BCB, 1, 0, -1.0, 1.0, 1, 0});
        gemm_step(1, 0);
      }
    }
    if (P.xrows) {
      CholStep s{};
      s.kind = CS_XROW_LAST, s.q = nb - 1, s.gy = 1;
      s.xa = CholXrowArg{nb - 1, 8 * (nb - 1 + (in.want_transpose ? 1 : 0)), 2};
      s.gx = std::min(batch * s.xa.nx, 2048);
      P.steps.push_back(s);
    }
    // (with the inverse formed from the parked panels nothing but a caller that reads L itself needs them moved below the diagonal)
    if (in.need_factor || !P.xrows) {
      CholStep s{};
      s.kind = CS_MIRROR, s.gx = std::min(1024, (n / 16) * (n / 16)), s.gy = batch;
      P.steps.push_back(s);
    }
  } else {
    CholStep s{};
    s.kind = CS_TRTRI_DIAG64, s.gx = nb * batch, s.gy = 1;
    P.steps.push_back(s);
  }
  if (in.want_inverse && !P.xrows) {
    // X = L^-1 by RECURSIVE DOUBLING over the diagonal inverses the factor kernel left on Linv's diagonal: at block size s every pair of
    // adjacent diagonal blocks [X11 0; X21 X22] gets X21 = -X22 (L21 X11), all n / 2s pairs (and all matrices of the batch) in ONE grouped
    // launch per product: 2 log2(n / 64) launches (8 at n = 1024) instead of the 2 (n / 64 - 1) of the block-row recurrence, and the upper
    // levels are big enough for the 128 x 128 kernel.  T = L21 X11 is parked in the mirror position of the X21 block inside S.
    for (int sblk = bs; sblk < n; sblk *= 2) {
      std::vector<CholGemm> l2;
      for (int r0 = sblk; r0 < n; r0 += 2 * sblk) {
        const int c0 = r0 - sblk, rows = std::min(n - r0, sblk);      // ragged last pair (n / 64 not a power of two)
        const CholRef l21{CB_W, r0 * N + c0}, x11{CB_LINV, c0 * N + c0}, t{CB_S, r0 * N + c0}, x22{CB_LINV, r0 * N + r0}, x21{CB_LINV, r0 * N + c0};
        P.gemms.push_back(CholGemm{l21, x11, t, rows, sblk, sblk, 0, 0, 1.0, 0.0, 0, 1});      // X11 lower-triangular: k >= n
        l2.push_back(CholGemm{x22, t, x21, rows, sblk, rows, 0, 0, -1.0, 0.0, 0, 2});          // X22 lower-triangular: k <= m
      }
      gemm_step((int)l2.size(), sblk <= 256 ? 0 : 1);      // short K: the 64 x 64 kernels
      P.gemms.insert(P.gemms.end(), l2.begin(), l2.end());
      gemm_step((int)l2.size(), sblk <= 256 ? 0 : 1);
    }
    if (in.want_transpose) {
      CholStep s{};
      s.kind = CS_TRANSPOSE, s.gx = 256, s.gy = batch;
      P.steps.push_back(s);
    }
  }
  bool uses_s = false;
  for (const CholGemm& g : P.gemms) uses_s = uses_s || g.C.buf == CB_S;
  P.tbuf_bytes = in.want_inverse || in.caller_tbuf ? 0 : (size_t)batch * P.stride[CB_TBUF] * sizeof(double);
  P.s_bytes = uses_s && !in.want_transpose ? (size_t)batch * P.stride[CB_S] * sizeof(double) : 0;
  P.items_bytes = in.from_tri ? (size_t)round_up((int64_t)nb * batch * CHOL_ITEM_BYTES, 256) : 0;
  P.desc_bytes = P.items_bytes + (size_t)round_up((int64_t)P.gemms.size() * CHOL_GEMM_BYTES, 256);
  return P;
}
