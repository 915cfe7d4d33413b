// Lloyd's k-means for the inducing points on the device: Z = kmeans2(X, M, minit='points')[0] of demos/run_regression.py:57, the one
// numeric step of the workflow the library did not cover.  One iteration = assign (every row to its nearest centre) + update (every
// centre to the mean of its rows); `iters` of them are enqueued on the context's stream without a host synchronisation.
//
// Centring.  k-means is translation-invariant; |x|^2 + |z|^2 - 2 x.z on data far from the origin is not (X = N(0, 1) + 1e6 loses
// 12 of fp64's 16 digits to |x|^2 ~ 1e12 before the distances of order 1 appear).  k_km_center subtracts the column means once;
// every distance and every centroid sum below is formed from the centred rows Xc, and the mean is added back when Z is written.
//
// Assign (k_km_assign, the hot path).  argmin_m |x_i - z_m|^2 = argmin_m (|z_m|^2 - 2 x_i.z_m); the cross products run on
// v_mfma_f64_16x16x4_f64 with the CENTRES as the A operand (matrix rows) and the data ROWS as the B operand (matrix columns), so a lane
// (g, c) holds, in the four registers of an accumulator, data row c against the centres g, g + 4, g + 8, g + 12 of a 16-centre fragment.
// A workgroup of four waves owns KM_BR = 128 rows; a wave owns 32 of them (two B fragments) against a tile of KM_BM = 64 centres
// (four A fragments): 8 accumulators, 8 MFMAs per 6 LDS reads.  Both operands are staged through LDS in k-chunks of KM_BK = 32
// (row stride 34 doubles: lane (g, c) reads double c*34 + g, the 32 lanes of an LDS cycle hit 32 different 8-byte banks); the next
// chunk's global loads are issued into registers before the current chunk's MFMAs and stored to LDS after them.  Per workgroup
// Z is read once and the X tile M / 64 times, all from L2: 3 M D 8 bytes for 2 128 M D flops = 10.7 flop per byte.
// After a centre tile's last chunk every lane folds its 4 x 4 x 2 values into a running (min, argmin) per data row with a strict <
// in ascending centre order; after the last tile the four g-groups of a row are combined (smaller value, then smaller index).  Nothing
// of size n x M is written.  Ties go to the lowest index; a NaN never wins, so a label always lies in [0, M).
//
// Update.  A stable counting sort of the row indices by label (k_km_hist: per-chunk histograms with integer LDS atomics; k_km_scan:
// the exclusive scan over (cluster, chunk); k_km_scatter: one wave per chunk walks its rows in order, same-label lanes ranked by
// ballot), then k_km_update: one workgroup per cluster sums its rows in ascending row order, TY interleaved partial sums per column
// combined by a fixed tree.  No floating-point atomics; the summation order depends on (n, D, M) and the labels alone.
// A cluster without rows keeps its centre (scipy's missing='warn'); one that never had rows returns Z0's bits.
#include <math.h>

#include "common.hpp"

#define KM_T 256
#define KM_BR 128      // data rows of a workgroup
#define KM_BM 64       // centres of a tile
#define KM_BK 32       // k-chunk staged in LDS
#define KM_LD 34       // LDS row stride in doubles
#define KM_XP (KM_BR * KM_BK / KM_T)      // doubles of the X chunk a thread stages (16)
#define KM_ZP (KM_BM * KM_BK / KM_T)      // ... of the Z chunk (8)
#define KM_MAX_M 2048
#define KM_MAX_D 1024
#define KM_SORT_ROWS 256      // smallest chunk of rows a sorting wave owns
#define KM_SORT_CHUNKS 512    // most chunks

// ---------------------------------------------------------------------------------------------------------------- centring
// partial[b][d] = sum of X[r][d] over the rows r of chunk b: thread (ty, tx) adds rows ty, ty + TY, ... of column tx (+ TX ...), the
// TY partial sums are combined in ascending ty
__global__ __launch_bounds__(KM_T) void k_km_colsum(const double* __restrict__ X, int64_t n, int D, int64_t rows_per_block, int TX,
                                                     double* __restrict__ partial) {
  __shared__ double red[KM_T];
  const int tid = threadIdx.x, TY = KM_T / TX, tx = tid % TX, ty = tid / TX;
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

__global__ __launch_bounds__(KM_T) void k_km_colmean(const double* __restrict__ partial, int nb, int D, int64_t n, double* __restrict__ mean) {
  const int d = blockIdx.x * KM_T + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(int64_t)b * D + d];
  mean[d] = s / (double)n;
}

// dst[r][d] = src[r][d] - mean[d], norm[r] = sum_d dst[r][d]^2.  G = 2^k lanes share a row (64 / G rows per wave): lane `sub` takes the
// columns sub, sub + G, ... in order, the G partial sums are combined by the xor butterfly (every lane ends with the same bits)
__global__ __launch_bounds__(KM_T) void k_km_center(const double* __restrict__ src, const double* __restrict__ mean, int64_t rows, int D,
                                                     int G, double* __restrict__ dst, double* __restrict__ norm) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rpw = 64 / G, sub = lane % G;
  const int64_t row = ((int64_t)blockIdx.x * (KM_T / 64) + w) * rpw + lane / G;
  const bool live = row < rows;
  double s = 0.0;
  if (live)
    for (int d = sub; d < D; d += G) {
      const double v = src[row * D + d] - mean[d];
      dst[row * D + d] = v;
      s = fma(v, v, s);
    }
  for (int off = G >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (live && sub == 0) norm[row] = s;
}

// ---------------------------------------------------------------------------------------------------------------- assign
struct KmStage {
  double x[KM_XP], z[KM_ZP];
};

// the chunk (m0, k0) of both operands into registers: thread -> column tid & 31, rows (tid >> 5) + 8 p.  Xc and Zc are padded with
// zero rows to whole tiles (the launcher), so only the columns need a guard: the load is issued from a clamped column and the zero
// selected afterwards — no branch around a load, one address per operand with a uniform stride between its loads
__device__ __forceinline__ void km_load(KmStage& s, const double* __restrict__ Xc, const double* __restrict__ Zc, int64_t r0, int D,
                                        int m0, int k0, int tid) {
  const int col = tid & 31, rr = tid >> 5;
  const int k = k0 + col;
  const bool kin = k < D;
  const double* px = Xc + (r0 + rr) * D + (kin ? k : D - 1);
  const double* pz = Zc + (int64_t)(m0 + rr) * D + (kin ? k : D - 1);
  const int step = 8 * D;
#pragma unroll
  for (int p = 0; p < KM_XP; ++p) {
    const double v = px[(int64_t)p * step];
    s.x[p] = kin ? v : 0.0;
  }
#pragma unroll
  for (int p = 0; p < KM_ZP; ++p) {
    const double v = pz[(int64_t)p * step];
    s.z[p] = kin ? v : 0.0;
  }
}

__device__ __forceinline__ void km_store(const KmStage& s, double* sX, double* sZ, int tid) {
  const int col = tid & 31, rr = tid >> 5;
#pragma unroll
  for (int p = 0; p < KM_XP; ++p) sX[(p * 8 + rr) * KM_LD + col] = s.x[p];
#pragma unroll
  for (int p = 0; p < KM_ZP; ++p) sZ[(p * 8 + rr) * KM_LD + col] = s.z[p];
}

__global__ __launch_bounds__(KM_T, 2) void k_km_assign(const double* __restrict__ Xc, const double* __restrict__ Zc,
                                                     const double* __restrict__ zn, const double* __restrict__ xn, int64_t n, int D, int M,
                                                     int* __restrict__ labels, double* __restrict__ dmin) {
  __shared__ double sX[KM_BR * KM_LD];
  __shared__ double sZ[KM_BM * KM_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = DS_WAVE_ID(tid);
  const int g = lane >> 4, c = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * KM_BR;
  const int nk = (D + KM_BK - 1) / KM_BK, nm = (M + KM_BM - 1) / KM_BM;
  const int stages = nk * nm;
  double best[2] = {INFINITY, INFINITY};
  int bidx[2] = {0, 0};
  d4 acc[4][2];
  const double* xa = sX + (w * 32 + c) * KM_LD + g;      // B operand: data row w*32 + rj*16 + c, k = kk + g
  const double* za = sZ + c * KM_LD + g;                 // A operand: centre mi*16 + c, k = kk + g
  KmStage st;
  km_load(st, Xc, Zc, r0, D, 0, 0, tid);
  for (int s = 0; s < stages; ++s) {
    const int mt = s / nk, kt = s - mt * nk;
    const int m0 = mt * KM_BM, k0 = kt * KM_BK;
    if (kt == 0) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int rj = 0; rj < 2; ++rj) acc[mi][rj] = d4{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();      // the previous chunk's LDS reads are done
    km_store(st, sX, sZ, tid);
    __syncthreads();
    if (s + 1 < stages) {
      const int mt1 = (s + 1) / nk, kt1 = (s + 1) - mt1 * nk;
      km_load(st, Xc, Zc, r0, D, mt1 * KM_BM, kt1 * KM_BK, tid);
    }
    const int kleft = D - k0;      // k-steps of 4 that hold a column (the rest of the chunk is zero on both sides)
    const int ksteps = kleft >= KM_BK ? KM_BK / 4 : (kleft + 3) >> 2;
    if (ksteps == KM_BK / 4) {
#pragma unroll
      for (int ks = 0; ks < KM_BK / 4; ++ks) {
        double a[4], b[2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) a[mi] = za[mi * 16 * KM_LD + ks * 4];
#pragma unroll
        for (int rj = 0; rj < 2; ++rj) b[rj] = xa[rj * 16 * KM_LD + ks * 4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int rj = 0; rj < 2; ++rj) acc[mi][rj] = mfma_f64(a[mi], b[rj], acc[mi][rj]);
      }
    } else {
      for (int ks = 0; ks < ksteps; ++ks) {
        double a[4], b[2];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) a[mi] = za[mi * 16 * KM_LD + ks * 4];
#pragma unroll
        for (int rj = 0; rj < 2; ++rj) b[rj] = xa[rj * 16 * KM_LD + ks * 4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int rj = 0; rj < 2; ++rj) acc[mi][rj] = mfma_f64(a[mi], b[rj], acc[mi][rj]);
      }
    }
    if (kt == nk - 1) {
      // accumulator (mi, rj), register t: centre m0 + mi*16 + g + 4t against data row rj*16 + c — ascending centres per lane
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int m = m0 + mi * 16 + g + 4 * t;
          const bool in = m < M;
          const double z2 = in ? zn[m] : 0.0;
#pragma unroll
          for (int rj = 0; rj < 2; ++rj) {
            const double v = fma(-2.0, acc[mi][rj][t], z2);
            if (in && v < best[rj]) {
              best[rj] = v;
              bidx[rj] = m;
            }
          }
        }
    }
  }
  // the four g-groups of a data row: the smaller value, on a tie the smaller index
#pragma unroll
  for (int rj = 0; rj < 2; ++rj) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const double ov = __shfl_xor(best[rj], off);
      const int oi = __shfl_xor(bidx[rj], off);
      if (ov < best[rj] || (ov == best[rj] && oi < bidx[rj])) {
        best[rj] = ov;
        bidx[rj] = oi;
      }
    }
    const int64_t row = r0 + w * 32 + rj * 16 + c;
    if (g == 0 && row < n) {
      labels[row] = bidx[rj];
      dmin[row] = fmax(best[rj] + xn[row], 0.0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- update
// hist[b][m] = rows of chunk b with label m (integer atomics in LDS: the counts do not depend on their order)
__global__ __launch_bounds__(KM_T) void k_km_hist(const int* __restrict__ labels, int64_t n, int M, int64_t chunk, int* __restrict__ hist) {
  __shared__ int h[KM_MAX_M];
  const int tid = threadIdx.x;
  for (int m = tid; m < M; m += KM_T) h[m] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
  for (int64_t r = r0 + tid; r < r1; r += KM_T) atomicAdd(&h[labels[r]], 1);
  __syncthreads();
  for (int m = tid; m < M; m += KM_T) hist[(int64_t)blockIdx.x * M + m] = h[m];
}

// one workgroup: hist[b][m] <- rows of label m in the chunks before b; cnt[m]; start[m] = rows of the labels before m (start[M] = n)
__global__ __launch_bounds__(1024) void k_km_scan(int* __restrict__ hist, int nb, int M, int* __restrict__ cnt, int* __restrict__ start) {
  __shared__ int tot[KM_MAX_M];
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  for (int m = tid; m < M; m += 1024) {
    int run = 0;
    for (int b = 0; b < nb; ++b) {
      const int v = hist[(int64_t)b * M + m];
      hist[(int64_t)b * M + m] = run;
      run += v;
    }
    tot[m] = run;
    cnt[m] = run;
  }
  __syncthreads();
  // exclusive scan of tot[0 .. M): thread t owns the entries 2t, 2t + 1
  const int a0 = 2 * tid < M ? tot[2 * tid] : 0, a1 = 2 * tid + 1 < M ? tot[2 * tid + 1] : 0;
  part[tid] = a0 + a1;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int before = part[tid] - (a0 + a1);
  if (2 * tid < M) start[2 * tid] = before;
  if (2 * tid + 1 < M) start[2 * tid + 1] = before + a0;
  if (tid == 1023) start[M] = part[1023];
}

// perm[start[m] + (rows of label m before r)] = r.  One wave per chunk, 64 rows at a time in row order: the lanes that share a label
// find each other by ballot, take consecutive slots from the label's cursor in lane order, and the last of them moves the cursor.
__global__ __launch_bounds__(64) void k_km_scatter(const int* __restrict__ labels, int64_t n, int M, int64_t chunk,
                                                   const int* __restrict__ hist, const int* __restrict__ start, int* __restrict__ perm) {
  __shared__ int cur[KM_MAX_M];
  const int lane = threadIdx.x;
  for (int m = lane; m < M; m += 64) cur[m] = start[m] + hist[(int64_t)blockIdx.x * M + m];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * chunk;
  const int64_t r1 = r0 + chunk < n ? r0 + chunk : n;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t base = r0; base < r1; base += 64) {
    const int64_t r = base + lane;
    const bool live = r < r1;
    const int lab = live ? labels[r] : -1;
    int rank = 0, total = 0;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int ll = __shfl(lab, lead);
      const unsigned long long same = __ballot(lab == ll);
      if (lab == ll) {
        rank = __popcll(same & below);
        total = __popcll(same);
      }
      todo &= ~same;
    }
    int pos = 0;
    if (live) pos = cur[lab] + rank;
    __syncthreads();
    if (live) {
      perm[pos] = (int)r;
      if (rank == total - 1) cur[lab] += total;
    }
    __syncthreads();
  }
}

// centre m <- mean of its rows (perm[start[m] .. start[m + 1]), ascending rows), zn[m] <- its squared norm; an empty cluster is left alone.
// Thread (ty, tx) adds the rows ty, ty + TY, ... of the segment for column tx (+ TX ...); the TY partial sums are combined in ascending ty.
__global__ __launch_bounds__(KM_T) void k_km_update(const double* __restrict__ Xc, const int* __restrict__ perm, const int* __restrict__ start,
                                                     int D, int TX, double* __restrict__ Zc, double* __restrict__ zn, int* __restrict__ ever) {
  __shared__ double red[KM_T];
  __shared__ double zrow[KM_MAX_D];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int s = start[m], e = start[m + 1];
  if (e == s) return;
  const int TY = KM_T / TX, tx = tid % TX, ty = tid / TX;
  const double cnt = (double)(e - s);
  for (int d0 = 0; d0 < D; d0 += TX) {
    const int d = d0 + tx;
    double sum = 0.0;
    if (d < D)
      for (int i = s + ty; i < e; i += TY) sum += Xc[(int64_t)perm[i] * D + d];
    red[tid] = sum;
    __syncthreads();
    if (ty == 0 && d < D) {
      double t = 0.0;
      for (int q = 0; q < TY; ++q) t += red[q * TX + tx];
      const double z = t / cnt;
      Zc[(int64_t)m * D + d] = z;
      zrow[d] = z;
    }
    __syncthreads();
  }
  double q = 0.0;
  for (int d = tid; d < D; d += KM_T) q = fma(zrow[d], zrow[d], q);
  q = block_sum<KM_T>(q, red);
  if (tid == 0) {
    zn[m] = q;
    ever[m] = 1;
  }
}

// Z[m][d] = Zc[m][d] + mean[d] for a centre that was averaged at least once, Z0's bits for one that never had rows (Z may alias Z0:
// every element is read and written by the same thread); counts as int64
__global__ __launch_bounds__(KM_T) void k_km_finish(const double* __restrict__ Zc, const double* __restrict__ mean, const int* __restrict__ ever,
                                                     const int* __restrict__ cnt, const double* Z0, int M, int D, double* Z,
                                                     int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * KM_T + threadIdx.x;
  if (i < (int64_t)M * D) {
    const int m = (int)(i / D), d = (int)(i - (int64_t)m * D);
    const double z0 = Z0[i];
    Z[i] = ever[m] ? Zc[i] + mean[d] : z0;
  }
  if (counts && i < M) counts[i] = cnt[i];
}

// inertia = sum_i dmin[i]: thread t adds the rows t, t + 1024, ... in order, then a fixed tree
__global__ __launch_bounds__(1024) void k_km_inertia(const double* __restrict__ dmin, int64_t n, double* __restrict__ out) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t r = tid; r < n; r += 1024) s += dmin[r];
  s = block_sum<1024>(s, red);
  if (tid == 0) out[0] = s;
}

static inline int km_pow2_lanes(int D, int lo) {      // the power of two >= min(D, 64), at least lo
  int g = lo;
  while (g < D && g < 64) g <<= 1;
  return g;
}

extern "C" int dsdgp_kmeans(dsdgp_ctx* ctx, const double* X, int64_t n, int32_t D, int32_t M, const double* Z0, int32_t iters, double* Z,
                            int32_t* labels, int64_t* counts, double* inertia) {
  DS_CHECK_ARG(ctx && X && Z0 && Z);
  DS_CHECK_ARG(M >= 2 && M <= KM_MAX_M);
  DS_CHECK_ARG(D >= 1 && D <= KM_MAX_D);
  DS_CHECK_ARG(n >= M && n <= 0x7fffffff);      // row indices are sorted as int32
  DS_CHECK_ARG(iters >= 1);
  hipStream_t st = ctx->stream;
  // chunks of the column sums (<= 1024) and of the counting sort (<= KM_SORT_CHUNKS): by (n) alone, so the bits do not depend on the device
  const int64_t sum_rows = round_up(ceil_div(n, 1024), 32);
  const int sum_nb = ceil_div(n, sum_rows);
  int64_t chunk = round_up(ceil_div(n, KM_SORT_CHUNKS), 64);
  if (chunk < KM_SORT_ROWS) chunk = KM_SORT_ROWS;
  const int nb = ceil_div(n, chunk);
  // scratch: doubles first, then the int32 arrays
  const size_t nd = (size_t)n * D, md = (size_t)M * D;
  // the assign launch reads whole tiles: Xc padded to KM_BR rows, Zc to KM_BM centres, the padding zeroed below
  const size_t ndp = (size_t)round_up(n, KM_BR) * D, mdp = (size_t)round_up(M, KM_BM) * D;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += (size_t)round_up((int64_t)bytes, 256); return at; };
  const size_t o_xc = take(ndp * 8), o_xn = take((size_t)n * 8), o_dmin = take((size_t)n * 8), o_zc = take(mdp * 8), o_zn = take((size_t)M * 8);
  const size_t o_mean = take((size_t)D * 8), o_part = take((size_t)sum_nb * D * 8), o_lab = take((size_t)n * 4), o_perm = take((size_t)n * 4);
  const size_t o_hist = take((size_t)nb * M * 4), o_start = take((size_t)(M + 1) * 4), o_cnt = take((size_t)M * 4), o_ever = take((size_t)M * 4);
  void* scr;
  DS_TRY(ctx_scratch(ctx, off, &scr));
  char* base = (char*)scr;
  double *Xc = (double*)(base + o_xc), *xn = (double*)(base + o_xn), *dmin = (double*)(base + o_dmin), *Zc = (double*)(base + o_zc);
  double *zn = (double*)(base + o_zn), *mean = (double*)(base + o_mean), *part = (double*)(base + o_part);
  int *lab = labels ? labels : (int*)(base + o_lab), *perm = (int*)(base + o_perm), *hist = (int*)(base + o_hist);
  int *start = (int*)(base + o_start), *cnt = (int*)(base + o_cnt), *ever = (int*)(base + o_ever);
  ProfScope prof(ctx, "kmeans");
  DS_HIP(hipMemsetAsync(ever, 0, (size_t)M * 4, st));
  if (ndp > nd) DS_HIP(hipMemsetAsync(Xc + nd, 0, (ndp - nd) * 8, st));
  if (mdp > md) DS_HIP(hipMemsetAsync(Zc + md, 0, (mdp - md) * 8, st));
  const int TX = km_pow2_lanes(D, 4), G = km_pow2_lanes(D, 1);
  const int rows_per_center_block = (KM_T / 64) * (64 / G);
  DS_LAUNCH(k_km_colsum, dim3(sum_nb), dim3(KM_T), 0, st, X, n, D, sum_rows, TX, part);
  DS_LAUNCH(k_km_colmean, dim3(ceil_div(D, KM_T)), dim3(KM_T), 0, st, part, sum_nb, D, n, mean);
  DS_LAUNCH(k_km_center, dim3(ceil_div(n, rows_per_center_block)), dim3(KM_T), 0, st, X, mean, n, D, G, Xc, xn);
  DS_LAUNCH(k_km_center, dim3(ceil_div(M, rows_per_center_block)), dim3(KM_T), 0, st, Z0, mean, (int64_t)M, D, G, Zc, zn);
  for (int it = 0; it < iters; ++it) {
    {
      ProfScope pa(ctx, "kmeans_assign");
      DS_LAUNCH(k_km_assign, dim3(ceil_div(n, KM_BR)), dim3(KM_T), 0, st, Xc, Zc, zn, xn, n, D, M, lab, dmin);
    }
    ProfScope pu(ctx, "kmeans_update");
    DS_LAUNCH(k_km_hist, dim3(nb), dim3(KM_T), 0, st, lab, n, M, chunk, hist);
    DS_LAUNCH(k_km_scan, dim3(1), dim3(1024), 0, st, hist, nb, M, cnt, start);
    DS_LAUNCH(k_km_scatter, dim3(nb), dim3(64), 0, st, lab, n, M, chunk, hist, start, perm);
    DS_LAUNCH(k_km_update, dim3(M), dim3(KM_T), 0, st, Xc, perm, start, D, TX, Zc, zn, ever);
  }
  DS_LAUNCH(k_km_finish, dim3(ceil_div((int64_t)md, KM_T)), dim3(KM_T), 0, st, Zc, mean, ever, cnt, Z0, M, D, Z, counts);
  if (inertia) DS_LAUNCH(k_km_inertia, dim3(1), dim3(1024), 0, st, dmin, n, inertia);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}
