// PCA for the step-down mean functions on the device: the top k right singular vectors of X (the np.linalg.svd step of the reference's
// init_layers_linear, layer_initializations.py:35) as the top k eigenvectors of the D x D matrix C = X^T X, D <= 1024.
//
// Gram (k_pca_gram, the hot path).  C = sum_r x_r x_r^T is a symmetric rank-n update: only the 64 x 64 tiles (I, J), I >= J, on or below
// the diagonal are formed, on v_mfma_f64_16x16x4_f64.  The reduction index is the ROW of X, so both operands are column slices of the same
// rows: a workgroup of four waves stages chunks of PG_BK = 32 rows x 64 columns for I and for J (one copy on a diagonal tile) in LDS, row
// stride PG_LD = 80 doubles — lane (g, c) of a fragment reads double g*80 + c, the 32 lanes of an LDS cycle (g = 0, 1) hit the 8-byte
// banks c and 16 + c — and a wave owns 32 x 32 of the tile (two A and two B fragments: 4 MFMAs per 4 LDS reads).  The next chunk's
// global loads are issued into registers before the current chunk's MFMAs and stored to LDS after them.  With center = 1 the column
// mean is subtracted when a chunk is staged (a thread stages one column, its mean sits in a register); X^T X - n m m^T is never formed.
// The rows are split over gridDim.y workgroups so that a launch has about PG_TARGET_WG of them whatever D is; a split writes its partial
// tile, k_pca_gram_reduce adds the partials in ascending split order and mirrors the result into the solver's matrix and `gram`
// (a diagonal tile is mirrored from its lower half, so C is exactly symmetric).  No floating-point atomics: the summation order
// depends on (n, D) alone.
//
// Eigensolver.  Two-sided Jacobi with the round-robin ordering: Dp = D padded to even (the padding row and column are zero and are never
// rotated), a sweep = Dp - 1 steps of Dp / 2 disjoint pairs, step s, pair m:  m = 0: (s, Dp - 1);  m >= 1: (s + m, s - m) mod (Dp - 1),
// smaller index first.  One launch per step (k_pca_step) reads A_in, V_in and writes A_out = J^T A_in J, V_out = V_in J: a thread owns
// the 2 x 2 block (pair a, pair b), b <= a, and writes it and its mirror image, so A stays exactly symmetric; every workgroup recomputes
// the rotations of its 16 + 16 pairs from A_in's diagonal blocks.  Pair (p, q) is skipped when |a_pq| <= 2^-53 sqrt(|a_pp a_qq|);
// otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with sgn(0) = 1 (a_pp = a_qq: 45 degrees),
// c = 1 / sqrt(t^2 + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0 exactly.  After a sweep k_pca_norm sums the squares of the
// off-diagonal entries themselves in a fixed order and sets the device flag when off <= D 2^-52 |C|_F or the sweep rotated nothing;
// every later step returns at once.  No kernel waits for another workgroup, the host enqueues max_sweeps sweeps and never waits.
// k_pca_rank orders the diagonal (rank of i = #{j: l_j > l_i, or l_j = l_i and j < i}), k_pca_gather writes the k leading columns of
// V with the entry of largest magnitude (ties: the lowest row) made positive.
#include <math.h>

#include "common.hpp"

#define PCA_MAX_D 1024
#define PCA_MAX_SWEEPS 64
#define PCA_SCRATCH_CAP ((size_t)256 << 20)      // bytes of split partials
#define PG_T 256
#define PG_BT 64            // tile edge of C
#define PG_BK 32            // rows of X per staged chunk
#define PG_LD 80            // LDS row stride in doubles
#define PG_P (PG_BK * PG_BT / PG_T)      // doubles of a chunk a thread stages per operand (8)
#define PG_TARGET_WG 1024
#define PG_MIN_ROWS 256     // fewest rows worth a split
#define PJ_B 16             // pairs per side of a step workgroup
#define PN_T 1024

// ---------------------------------------------------------------------------------------------------------------- column means
// partial[b][d] = sum of X[r][d] over the rows r of chunk b: thread (ty, tx) adds rows ty, ty + TY, ... of column tx (+ TX ...), the
// TY partial sums are combined in ascending ty
__global__ __launch_bounds__(PG_T) void k_pca_colsum(const double* __restrict__ X, int64_t n, int D, int64_t rows_per_block, int TX,
                                                     double* __restrict__ partial) {
  __shared__ double red[PG_T];
  const int tid = threadIdx.x, TY = PG_T / TX, tx = tid % TX, ty = tid / TX;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  for (int d0 = 0; d0 < D; d0 += TX) {
    const int d = d0 + tx;
    double s = 0.0;
    if (d < D)
      for (int64_t r = r0 + ty; r < r1; r += TY) s += X[r * D + d];
    red[tid] = s;
    __syncthreads();
    if (ty == 0 && d < D) {
      double t = 0.0;
      for (int q = 0; q < TY; ++q) t += red[q * TX + tx];
      partial[(int64_t)blockIdx.x * D + d] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PG_T) void k_pca_colmean(const double* __restrict__ partial, int nb, int D, int64_t n, double* __restrict__ mean) {
  const int d = blockIdx.x * PG_T + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(int64_t)b * D + d];
  mean[d] = s / (double)n;
}

// ---------------------------------------------------------------------------------------------------------------- Gram
// rows [r, r + PG_BK) x columns [c0, c0 + 64) of X - mean into registers: thread -> column tid & 63, rows (tid >> 6) + 4 p.  Rows past
// `rend` and columns past D are loaded from a clamped address and replaced by zero afterwards — no branch around a load
__device__ __forceinline__ void pg_load(double (&v)[PG_P], const double* __restrict__ X, int64_t r, int64_t rend, int D, int c0, double m,
                                        int tid) {
  const int col = c0 + (tid & 63), rr = tid >> 6;
  const bool cin = col < D;
  const double* px = X + (cin ? col : D - 1);
#pragma unroll
  for (int p = 0; p < PG_P; ++p) {
    const int64_t row = r + rr + 4 * p;
    const bool in = cin && row < rend;
    const double x = px[(row < rend ? row : rend - 1) * D];
    v[p] = in ? x - m : 0.0;
  }
}

__device__ __forceinline__ void pg_store(const double (&v)[PG_P], double* s, int tid) {
  const int col = tid & 63, rr = tid >> 6;
#pragma unroll
  for (int p = 0; p < PG_P; ++p) s[(rr + 4 * p) * PG_LD + col] = v[p];
}

// tile t of the lower triangle -> (I, J), I >= J
__device__ __forceinline__ void pg_tile(int t, int& I, int& J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  J = t - I * (I + 1) / 2;
}

// part[(split * ntiles + tile) * 64 * 64 + i * 64 + j] = sum over the split's rows of Xc[r][I 64 + i] Xc[r][J 64 + j]
__global__ __launch_bounds__(PG_T, 2) void k_pca_gram(const double* __restrict__ X, const double* __restrict__ mean, int64_t n, int D,
                                                      int64_t rows_per_split, double* __restrict__ part) {
  __shared__ double sI[PG_BK * PG_LD];
  __shared__ double sJ[PG_BK * PG_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = DS_WAVE_ID(tid);
  const int g = lane >> 4, c = lane & 15;
  int I, J;
  pg_tile(blockIdx.x, I, J);
  const bool diag = I == J;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
  const int64_t r1 = r0 + rows_per_split < n ? r0 + rows_per_split : n;
  const int nchunk = (int)((r1 - r0 + PG_BK - 1) / PG_BK);
  const int colI = I * PG_BT + (tid & 63), colJ = J * PG_BT + (tid & 63);
  const double mI = mean && colI < D ? mean[colI] : 0.0, mJ = mean && colJ < D ? mean[colJ] : 0.0;
  const int wi = w >> 1, wj = w & 1;
  const double* pa = sI + g * PG_LD + wi * 32 + c;                     // A operand: column I 64 + wi 32 + ai 16 + c, row kk + g
  const double* pb = (diag ? sI : sJ) + g * PG_LD + wj * 32 + c;       // B operand: column J 64 + wj 32 + bj 16 + c, row kk + g
  d4 acc[2][2];
#pragma unroll
  for (int ai = 0; ai < 2; ++ai)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) acc[ai][bj] = d4{0.0, 0.0, 0.0, 0.0};
  double vi[PG_P], vj[PG_P];
  pg_load(vi, X, r0, r1, D, I * PG_BT, mI, tid);
  if (!diag) pg_load(vj, X, r0, r1, D, J * PG_BT, mJ, tid);
  for (int ch = 0; ch < nchunk; ++ch) {
    __syncthreads();      // the previous chunk's LDS reads are done
    pg_store(vi, sI, tid);
    if (!diag) pg_store(vj, sJ, tid);
    __syncthreads();
    if (ch + 1 < nchunk) {
      const int64_t r = r0 + (int64_t)(ch + 1) * PG_BK;
      pg_load(vi, X, r, r1, D, I * PG_BT, mI, tid);
      if (!diag) pg_load(vj, X, r, r1, D, J * PG_BT, mJ, tid);
    }
#pragma unroll
    for (int ks = 0; ks < PG_BK / 4; ++ks) {
      double a[2], b[2];
#pragma unroll
      for (int ai = 0; ai < 2; ++ai) a[ai] = pa[ks * 4 * PG_LD + ai * 16];
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) b[bj] = pb[ks * 4 * PG_LD + bj * 16];
#pragma unroll
      for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[ai][bj] = mfma_f64(a[ai], b[bj], acc[ai][bj]);
    }
  }
  // accumulator (ai, bj), register t: tile row wi 32 + ai 16 + g + 4t, tile column wj 32 + bj 16 + c
  double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PG_BT * PG_BT);
#pragma unroll
  for (int ai = 0; ai < 2; ++ai)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int t = 0; t < 4; ++t) out[(wi * 32 + ai * 16 + g + 4 * t) * PG_BT + wj * 32 + bj * 16 + c] = acc[ai][bj][t];
}

// C[i][j] = C[j][i] = sum of the partials in ascending split order, for the entries i >= j of the lower tiles; written to the solver's
// Dp x Dp matrix A and, if asked for, to the D x D `gram`
__global__ __launch_bounds__(PG_T) void k_pca_gram_reduce(const double* __restrict__ part, int nsplit, int ntiles, int D, int Dp,
                                                          double* __restrict__ A, double* __restrict__ gram) {
  int I, J;
  pg_tile(blockIdx.x, I, J);
  const int e = blockIdx.y * PG_T + threadIdx.x;      // entry of the tile
  const int li = e / PG_BT, lj = e - li * PG_BT;
  const int i = I * PG_BT + li, j = J * PG_BT + lj;
  if (i >= D || j > i) return;
  const double* p = part + (int64_t)blockIdx.x * (PG_BT * PG_BT) + e;
  double s = 0.0;
  for (int b = 0; b < nsplit; ++b) s += p[(int64_t)b * ntiles * (PG_BT * PG_BT)];
  A[(int64_t)i * Dp + j] = s;
  A[(int64_t)j * Dp + i] = s;
  if (gram) {
    gram[(int64_t)i * D + j] = s;
    gram[(int64_t)j * D + i] = s;
  }
}

__global__ __launch_bounds__(PG_T) void k_pca_eye(double* __restrict__ V, int Dp) {
  const int i = blockIdx.x * PG_T + threadIdx.x;
  if (i < Dp) V[(int64_t)i * Dp + i] = 1.0;
}

// ---------------------------------------------------------------------------------------------------------------- Jacobi
// ist: {converged, sweeps run, rotations of the last sweep, rotations of the sweep under way};  dst[0] = |C|_F
__device__ __forceinline__ void pj_pair(int m, int step, int Dp, int& p, int& q) {
  int a, b;
  if (m == 0) {
    a = step;
    b = Dp - 1;
  } else {
    a = (step + m) % (Dp - 1);
    b = (step - m + Dp - 1) % (Dp - 1);
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// grid (nb, 2 nb), nb = ceil(Dp / 2 / 16).  blockIdx.y < nb: the 2 x 2 blocks (pair a of block y, pair b of block x), b <= a, of
// A_out = J^T A_in J and their mirror images.  blockIdx.y >= nb: rows 2a, 2a + 1 of V_out = V_in J (the same arithmetic with the
// identity on the left)
__global__ __launch_bounds__(PJ_B* PJ_B) void k_pca_step(const double* __restrict__ Ain, double* __restrict__ Aout,
                                                         const double* __restrict__ Vin, double* __restrict__ Vout, int Dp, int step, int nb,
                                                         int* __restrict__ ist) {
  if (ist[0]) return;
  const bool isV = (int)blockIdx.y >= nb;
  const int by = isV ? blockIdx.y - nb : blockIdx.y, bx = blockIdx.x;
  if (!isV && bx > by) return;
  __shared__ double sc[2][PJ_B], ss[2][PJ_B], stn[2][PJ_B];
  __shared__ int sp[2][PJ_B], sq[2][PJ_B], srot[2][PJ_B];
  const int tid = threadIdx.x, half = Dp >> 1;
  if (tid < 2 * PJ_B) {
    const int which = tid >> 4, l = tid & 15;
    const int m = (which == 0 ? by : bx) * PJ_B + l;
    double cc = 1.0, sn = 0.0, tn = 0.0;
    int p = 0, q = 0, rot = 0;
    if (m < half && !(isV && which == 0)) {
      pj_pair(m, step, Dp, p, q);
      const double app = Ain[(int64_t)p * Dp + p], aqq = Ain[(int64_t)q * Dp + q], apq = Ain[(int64_t)p * Dp + q];
      if (!(fabs(apq) <= 0x1p-53 * sqrt(fabs(app * aqq)))) {
        const double theta = (aqq - app) / (2.0 * apq);
        tn = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        cc = 1.0 / sqrt(tn * tn + 1.0);
        sn = tn * cc;
        rot = 1;
      }
    }
    sc[which][l] = cc;
    ss[which][l] = sn;
    stn[which][l] = tn;
    sp[which][l] = p;
    sq[which][l] = q;
    srot[which][l] = rot;
  }
  __syncthreads();
  const int ta = tid >> 4, tb = tid & 15;
  const int ma = by * PJ_B + ta, mb = bx * PJ_B + tb;
  if (ma >= half || mb >= half) return;
  const int pb = sp[1][tb], qb = sq[1][tb];
  const double cb = sc[1][tb], sb = ss[1][tb];
  if (isV) {
    const int64_t r0 = (int64_t)(2 * ma) * Dp, r1 = r0 + Dp;
    const double v00 = Vin[r0 + pb], v01 = Vin[r0 + qb], v10 = Vin[r1 + pb], v11 = Vin[r1 + qb];
    Vout[r0 + pb] = cb * v00 - sb * v01;
    Vout[r0 + qb] = sb * v00 + cb * v01;
    Vout[r1 + pb] = cb * v10 - sb * v11;
    Vout[r1 + qb] = sb * v10 + cb * v11;
    return;
  }
  if (mb > ma) return;
  const int pa = sp[0][ta], qa = sq[0][ta];
  const int64_t ra = (int64_t)pa * Dp, rq = (int64_t)qa * Dp;
  if (mb == ma) {
    const double app = Ain[ra + pa], aqq = Ain[rq + qa], apq = Ain[ra + qa];
    const bool rot = srot[0][ta] != 0;
    const double tn = stn[0][ta];
    Aout[ra + pa] = rot ? app - tn * apq : app;
    Aout[rq + qa] = rot ? aqq + tn * apq : aqq;
    Aout[ra + qa] = rot ? 0.0 : apq;
    Aout[rq + pa] = rot ? 0.0 : apq;
    if (rot) atomicAdd(&ist[3], 1);      // an integer count: its value does not depend on the order
    return;
  }
  const double ca = sc[0][ta], sa = ss[0][ta];
  const double b00 = Ain[ra + pb], b01 = Ain[ra + qb], b10 = Ain[rq + pb], b11 = Ain[rq + qb];
  const double r00 = ca * b00 - sa * b10, r01 = ca * b01 - sa * b11;
  const double r10 = sa * b00 + ca * b10, r11 = sa * b01 + ca * b11;
  const double o00 = cb * r00 - sb * r01, o01 = sb * r00 + cb * r01;
  const double o10 = cb * r10 - sb * r11, o11 = sb * r10 + cb * r11;
  Aout[ra + pb] = o00;
  Aout[ra + qb] = o01;
  Aout[rq + pb] = o10;
  Aout[rq + qb] = o11;
  Aout[(int64_t)pb * Dp + pa] = o00;
  Aout[(int64_t)qb * Dp + pa] = o01;
  Aout[(int64_t)pb * Dp + qa] = o10;
  Aout[(int64_t)qb * Dp + qa] = o11;
}

// one workgroup.  sweep = 0: dst[0] = |C|_F.  sweep >= 1 (after that sweep; A is the buffer the sweep ended in): off = sqrt(sum of the
// squares of the off-diagonal entries) — thread t adds the entries t, t + 1024, ... in order, then a fixed tree — and the bookkeeping
__global__ __launch_bounds__(PN_T) void k_pca_norm(const double* __restrict__ A, int Dp, int D, int sweep, double* __restrict__ dst,
                                                   int* __restrict__ ist) {
  if (sweep > 0 && ist[0]) return;
  __shared__ double red[PN_T];
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)Dp * Dp;
  double s = 0.0;
  for (int64_t e = tid; e < total; e += PN_T) {
    const int i = (int)(e / Dp), j = (int)(e - (int64_t)i * Dp);
    const double a = A[e];
    if (sweep == 0 || i != j) s = fma(a, a, s);
  }
  s = block_sum<PN_T>(s, red);
  if (tid != 0) return;
  const double nrm = sqrt(s);
  if (sweep == 0) {
    dst[0] = nrm;
    return;
  }
  const int rot = ist[3];
  ist[1] = sweep;
  ist[2] = rot;
  ist[3] = 0;
  if (nrm <= (double)D * 0x1p-52 * dst[0] || rot == 0) ist[0] = 1;
}

// the final matrices are in buffer (sweeps run) & 1: a sweep has an odd number of steps
__global__ __launch_bounds__(PG_T) void k_pca_rank(const double* __restrict__ A0, const double* __restrict__ A1, int D, int Dp,
                                                   const int* __restrict__ ist, double* __restrict__ evals, int* __restrict__ order,
                                                   int32_t* __restrict__ info) {
  const double* A = (ist[1] & 1) ? A1 : A0;
  const int i = blockIdx.x * PG_T + threadIdx.x;
  if (i == 0 && info) {
    info[0] = ist[0];
    info[1] = ist[1];
    info[2] = ist[2];
    info[3] = 0;
  }
  if (i >= D) return;
  const double li = A[(int64_t)i * Dp + i];
  int rank = 0;
  for (int j = 0; j < D; ++j) {
    const double lj = A[(int64_t)j * Dp + j];
    rank += (lj > li || (lj == li && j < i)) ? 1 : 0;
  }
  order[rank] = i;
  if (evals) evals[rank] = li;
}

// W[:, j] = +- V[:, order[j]], the entry of largest magnitude positive (ties: the lowest row)
__global__ __launch_bounds__(PG_T) void k_pca_gather(const double* __restrict__ V0, const double* __restrict__ V1, int D, int Dp,
                                                     const int* __restrict__ ist, const int* __restrict__ order, double* __restrict__ W,
                                                     int64_t ldw) {
  __shared__ double rv[PG_T];
  __shared__ int ri[PG_T];
  const double* V = (ist[1] & 1) ? V1 : V0;
  const int j = blockIdx.x, tid = threadIdx.x, src = order[j];
  double best = -1.0;
  int bi = 0;
  for (int i = tid; i < D; i += PG_T) {
    const double a = fabs(V[(int64_t)i * Dp + src]);
    if (a > best) {
      best = a;
      bi = i;
    }
  }
  rv[tid] = best;
  ri[tid] = bi;
  __syncthreads();
  for (int h = PG_T / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      const double ov = rv[tid + h];
      const int oi = ri[tid + h];
      if (ov > rv[tid] || (ov == rv[tid] && oi < ri[tid])) {
        rv[tid] = ov;
        ri[tid] = oi;
      }
    }
    __syncthreads();
  }
  const double sgn = V[(int64_t)ri[0] * Dp + src] < 0.0 ? -1.0 : 1.0;
  for (int i = tid; i < D; i += PG_T) W[(int64_t)i * ldw + j] = sgn * V[(int64_t)i * Dp + src];
}

static inline int pca_pow2_lanes(int D) {      // the power of two >= min(D, 64), at least 4
  int g = 4;
  while (g < D && g < 64) g <<= 1;
  return g;
}

extern "C" int dsdgp_pca(dsdgp_ctx* ctx, const double* X, int64_t n, int32_t D, int32_t k, int32_t center, int32_t max_sweeps, double* W,
                         int64_t ldw, double* evals, double* mean, double* gram, int32_t* info) {
  DS_CHECK_ARG(ctx && X && W);
  DS_CHECK_ARG(n >= 1 && n <= 0x7fffffff);
  DS_CHECK_ARG(D >= 1 && D <= PCA_MAX_D);
  DS_CHECK_ARG(k >= 1 && k <= D);
  DS_CHECK_ARG(center == 0 || center == 1);
  DS_CHECK_ARG(max_sweeps >= 1 && max_sweeps <= PCA_MAX_SWEEPS);
  DS_CHECK_ARG(ldw >= k);
  hipStream_t st = ctx->stream;
  const int Dp = (D + 1) & ~1, half = Dp / 2;
  // the row splits of the Gram and the chunks of the column sums: by (n, D) alone, so the bits do not depend on the device
  const int nt1 = ceil_div(D, PG_BT), ntiles = nt1 * (nt1 + 1) / 2;
  const size_t tile_bytes = (size_t)ntiles * PG_BT * PG_BT * 8;
  int64_t want = ceil_div(PG_TARGET_WG, ntiles);
  const int64_t most = ceil_div(n, PG_MIN_ROWS);
  if (want > most) want = most;
  if (want > (int64_t)(PCA_SCRATCH_CAP / tile_bytes)) want = (int64_t)(PCA_SCRATCH_CAP / tile_bytes);
  if (want < 1) {
    dsdgp_set_error("%s:%d: one split's partial tiles (%zu bytes) exceed the cap of %zu", __FILE__, __LINE__, tile_bytes, PCA_SCRATCH_CAP);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const int64_t rows_per_split = round_up(ceil_div(n, want), PG_BK);
  const int nsplit = ceil_div(n, rows_per_split);
  const int64_t sum_rows = round_up(ceil_div(n, 1024), 32);
  const int sum_nb = ceil_div(n, sum_rows);
  const size_t dd = (size_t)Dp * Dp * 8;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (size_t)round_up((int64_t)bytes, 256); return at; };
  const size_t o_a0 = take(dd), o_a1 = take(dd), o_v0 = take(dd), o_v1 = take(dd), o_part = take((size_t)nsplit * tile_bytes);
  const size_t o_mean = take((size_t)D * 8), o_sum = take((size_t)sum_nb * D * 8), o_dst = take(8), o_ist = take(16);
  const size_t o_order = take((size_t)D * 4);
  void* scr;
  DS_TRY(ctx_scratch(ctx, off, &scr));
  char* base = (char*)scr;
  double *A0 = (double*)(base + o_a0), *A1 = (double*)(base + o_a1), *V0 = (double*)(base + o_v0), *V1 = (double*)(base + o_v1);
  double *part = (double*)(base + o_part), *sums = (double*)(base + o_sum), *dst = (double*)(base + o_dst);
  double* mu = mean ? mean : (double*)(base + o_mean);
  int *ist = (int*)(base + o_ist), *order = (int*)(base + o_order);
  ProfScope prof(ctx, "pca");
  DS_HIP(hipMemsetAsync(ist, 0, 16, st));
  DS_HIP(hipMemsetAsync(order, 0, (size_t)D * 4, st));      // a NaN on the diagonal leaves ranks unassigned: they then name column 0
  DS_HIP(hipMemsetAsync(A0, 0, dd, st));
  DS_HIP(hipMemsetAsync(V0, 0, dd, st));
  if (center) {
    DS_LAUNCH(k_pca_colsum, dim3(sum_nb), dim3(PG_T), 0, st, X, n, D, sum_rows, pca_pow2_lanes(D), sums);
    DS_LAUNCH(k_pca_colmean, dim3(ceil_div(D, PG_T)), dim3(PG_T), 0, st, sums, sum_nb, D, n, mu);
  } else if (mean) {
    DS_HIP(hipMemsetAsync(mean, 0, (size_t)D * 8, st));
  }
  {
    ProfScope pg(ctx, "pca_gram");
    DS_LAUNCH(k_pca_gram, dim3(ntiles, nsplit), dim3(PG_T), 0, st, X, center ? (const double*)mu : (const double*)nullptr, n, D,
              rows_per_split, part);
  }
  DS_LAUNCH(k_pca_gram_reduce, dim3(ntiles, PG_BT * PG_BT / PG_T), dim3(PG_T), 0, st, part, nsplit, ntiles, D, Dp, A0, gram);
  DS_LAUNCH(k_pca_eye, dim3(ceil_div(Dp, PG_T)), dim3(PG_T), 0, st, V0, Dp);
  {
    ProfScope ps(ctx, "pca_eig");
    DS_LAUNCH(k_pca_norm, dim3(1), dim3(PN_T), 0, st, A0, Dp, D, 0, dst, ist);
    const int nb = ceil_div(half, PJ_B);
    double *Ain = A0, *Aout = A1, *Vin = V0, *Vout = V1;
    for (int sweep = 1; sweep <= max_sweeps; ++sweep) {
      for (int step = 0; step < Dp - 1; ++step) {
        DS_LAUNCH(k_pca_step, dim3(nb, 2 * nb), dim3(PJ_B * PJ_B), 0, st, Ain, Aout, Vin, Vout, Dp, step, nb, ist);
        double* t = Ain; Ain = Aout; Aout = t;
        t = Vin; Vin = Vout; Vout = t;
      }
      DS_LAUNCH(k_pca_norm, dim3(1), dim3(PN_T), 0, st, Ain, Dp, D, sweep, dst, ist);
    }
  }
  DS_LAUNCH(k_pca_rank, dim3(ceil_div(D, PG_T)), dim3(PG_T), 0, st, A0, A1, D, Dp, ist, evals, order, info);
  DS_LAUNCH(k_pca_gather, dim3(k), dim3(PG_T), 0, st, V0, V1, D, Dp, ist, order, W, ldw);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}
