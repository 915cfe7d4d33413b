// What the reductions over the S mixture components of the (S, n, DY) last-layer means and variances share (evaluate.hip, calibration.hip,
// classification.hip):
// items -> threads, the sums over an item's lanes and per output, the second-stage kernel, the launch geometry.  Their math stays with them.
#pragma once
#include <type_traits>

#include "common.hpp"

#define MIX_T 256         // threads of a workgroup

// Threads map to consecutive flat (i, d) items, SPLIT adjacent lanes per item: lane `sub` of item `jl` of the workgroup takes the
// components s = sub, sub + SPLIT, ...  (SPLIT = 1: one thread per item, every s one coalesced row of loads).
template <int SPLIT>
struct MixItem {
  static constexpr int JPB = MIX_T / SPLIT;      // items of a workgroup
  const int sub = threadIdx.x % SPLIT, jl = threadIdx.x / SPLIT;
  const int64_t j0 = (int64_t)blockIdx.x * JPB;      // the workgroup's first item
  const bool live;
  const int64_t jc;      // this thread's item, the last one for the lanes past it  (every lane takes part in the folds)
  __device__ __forceinline__ explicit MixItem(int64_t total) : live(j0 + jl < total), jc(live ? j0 + jl : total - 1) {}
};

// the sum over the SPLIT adjacent lanes that share an item (butterfly; both partners evaluate the same expression, so every lane of
// the group ends with the same bits)
template <int SPLIT>
__device__ __forceinline__ double fold_sum(double x, int sub) {
#pragma unroll
  for (int off = 1; off < SPLIT; off <<= 1) {
    const double o = __shfl_xor(x, off);
    x = (sub & off) ? o + x : x + o;
  }
  return x;
}

// output d's sum of val(e) over the items e in [lo, hi) of a workgroup that starts at flat item j0, in ascending order: item e belongs
// to output (j0 + e) % ND
template <class F>
__device__ __forceinline__ double sum_output_items(int d, int ND, int64_t j0, int lo, int hi, F val) {
  double t = 0.0;
  for (int e = lo + (int)(((int64_t)d + ND - (j0 + lo) % ND) % ND); e < hi; e += ND) t += val(e);
  return t;
}

// second stage: acc[q DY + d] (+)= sum over the workgroups' partials part[q DY + d][block], one wave per entry: lane-strided partial
// sums, then the wave sum (both in a fixed order for a given number of workgroups).  Entries with d >= ND have no sums of their own and
// are zeroed.
static __global__ __launch_bounds__(MIX_T) void k_mixture_finish(const double* __restrict__ part, int nblocks, int entries, int DY, int ND,
                                                                 int accumulate, double* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wave = DS_WAVE_ID(threadIdx.x);
  for (int p = blockIdx.x * (MIX_T / 64) + wave; p < entries; p += gridDim.x * (MIX_T / 64)) {
    double t = 0.0;
    if (p % DY < ND)
      for (int b = lane; b < nblocks; b += 64) t += part[(int64_t)p * nblocks + b];
    t = sum_wave(t);
    if (lane == 0) acc[p] = accumulate ? acc[p] + t : t;
  }
}
static inline void mixture_finish_launch(hipStream_t st, const double* part, int nblocks, int entries, int DY, int ND, int accumulate,
                                         double* acc) {
  DS_LAUNCH(k_mixture_finish, dim3(ceil_div(entries, MIX_T / 64)), dim3(MIX_T), 0, st, part, nblocks, entries, DY, ND, accumulate, acc);
}

// Lanes per item by the item count: one while the items alone fill the chip (256 CUs x 2048 threads = 2^19 resident lanes at most; 2^15
// items already keep every CU busy), else 4, 8 or 16 so that a batch of ~1000 rows still spreads over the CUs ...
static inline int mix_split_by_items(int64_t total) { return total >= 32768 ? 1 : total >= 8192 ? 4 : total >= 4096 ? 8 : 16; }
// ... and never more lanes than components
static inline int mix_split_clamp(int split, int S) { while (split > 1 && split > S) split = (split == 4) ? 1 : split / 2; return split; }

// f(std::integral_constant<int, SPLIT>) for the run-time lanes per item
template <class F>
static inline void mix_dispatch_split(int split, F f) {
  if (split == 16) f(std::integral_constant<int, 16>());
  else if (split == 8) f(std::integral_constant<int, 8>());
  else if (split == 4) f(std::integral_constant<int, 4>());
  else f(std::integral_constant<int, 1>());
}

// workgroups of a launch over `total` items
static inline int mix_nblocks(int64_t total, int split, int* nblocks) {
  const int64_t nb64 = (total + MIX_T / split - 1) / (MIX_T / split);
  DS_CHECK_ARG(nb64 <= 0x7fffffff);
  *nblocks = (int)nb64;
  return DSDGP_OK;
}
