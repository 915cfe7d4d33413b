// Shared host/device helpers of libdsdgp (gfx950 / CDNA4 only; fp64 throughout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <map>

#include "../../include/dsdgp.h"

// ------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------
void dsdgp_set_error(const char* fmt, ...);

#define DS_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      dsdgp_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
      return DSDGP_ERR_HIP;                                                                  \
    }                                                                                        \
  } while (0)

#define DS_CHECK_ARG(cond)                                                  \
  do {                                                                      \
    if (!(cond)) {                                                          \
      dsdgp_set_error("%s:%d: bad argument: %s", __FILE__, __LINE__, #cond); \
      return DSDGP_ERR_BAD_ARG;                                             \
    }                                                                       \
  } while (0)

// every kernel launch of the library goes through this: a process-wide count of launches (dsdgp_launch_count: launches per step in
// bench.py's line; a relaxed atomic add, nothing else)
#include <atomic>
extern std::atomic<long long> g_dsdgp_launches;
#define DS_LAUNCH(...)                                                   \
  do {                                                                   \
    g_dsdgp_launches.fetch_add(1, std::memory_order_relaxed);            \
    hipLaunchKernelGGL(__VA_ARGS__);                                     \
  } while (0)

#define DS_TRY(call)            \
  do {                          \
    int rc__ = (call);          \
    if (rc__ != DSDGP_OK) return rc__; \
  } while (0)

// ------------------------------------------------------------------------------------------------------
// context: one per (host thread, device); owns the stream (unless borrowed) and a grow-only scratch used by the
// *primitive* entry points only (the model path runs entirely inside the caller's workspace).
// ------------------------------------------------------------------------------------------------------
struct ProfSlot {
  double ms = 0.0;
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct dsdgp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t side = nullptr;      // second stream of the models of this context (created with the first model)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  int prof_on = 0;
  std::map<std::string, ProfSlot> prof;
  // pinned staging ring for the small host->device descriptor uploads of the primitive entry points (kernel hyper-parameters,
  // GEMM / factorisation descriptors): the copy is enqueued from pinned memory and the call returns — no stream synchronisation
  char* pin = nullptr;
  size_t pin_bytes = 0, pin_off = 0;
  // dsdgp_potrf, n >= 512: the blocked factorisation's plan (descriptor arrays + scratch on the device) of the last call, reused
  // while matrix order, batch and scratch address repeat (a plan build costs two hipMallocs and a synchronous upload: ~150 us)
  void* potrf_plan = nullptr;
  void (*potrf_plan_free)(void*) = nullptr;
  int64_t potrf_key[4] = {0, 0, 0, 0};
};

int ctx_scratch(dsdgp_ctx* ctx, size_t bytes, void** out);
// asynchronous upload of a small host object to device memory `dst` on the ctx stream (the host copy may die on return)
int ctx_upload(dsdgp_ctx* ctx, void* dst, const void* src, size_t bytes);

// launchers that one translation unit defines and others call
int multiclass_launch(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n, int64_t R, int K,
                      int mode, double wgt, double* out, double* dmean, double* dvar, int y_override);      // multiclass.hip
// p0_dev / noise_dev != NULL: the likelihood's positive parameter is read on the device (a model's own copy); p0 / noise_var is ignored
int eval_mixture_launch(dsdgp_ctx* ctx, int kind, double p0, double p1, const double* p0_dev, const double* mean, const double* var,
                        const double* Y, int64_t n, int S, int DY, double* rows_out, double* acc, int accumulate);      // evaluate.hip
int mixture_quantiles_launch(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* noise_dev,
                             int64_t n, int S, int DY, const double* probs, int P, double* q_out);      // calibration.hip
int mixture_calibration_launch(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* noise_dev,
                               const double* Y, int64_t n, int S, int DY, const double* probs, int P, double* rows_out, double* acc,
                               int accumulate);
int mixture_classification_launch(dsdgp_ctx* ctx, int kind, const double* mean, const double* var, const double* Y, int64_t n, int S,
                                  int DY, int bins, double* probs_out, double* rows_out, double* acc, int accumulate);      // classification.hip

// RAII-ish profiling bracket: records HIP events on the ctx stream around a launch when profiling is enabled.
struct ProfScope {
  dsdgp_ctx* ctx;
  const char* name;
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st;
  ProfScope(dsdgp_ctx* c, const char* n, hipStream_t stream = nullptr) : ctx(c), name(n), st(stream ? stream : c->stream) {
    if (ctx->prof_on) {
      hipEventCreate(&a);
      hipEventCreate(&b);
      hipEventRecord(a, st);
    }
  }
  ~ProfScope() {
    if (a) {
      hipEventRecord(b, st);
      ctx->prof[name].pending.push_back({a, b});
    }
  }
};

// A thread's wave index is the same in all 64 lanes of its wave, but `threadIdx.x >> 6` is a per-lane value to the compiler: loops whose
// bounds depend on it (the triangular k ranges of the chains, the row ranges of the split-K products) become DIVERGENT loops — exec-mask
// loop control, no unrolling (the "loop not unrolled" warnings), 64-bit VALU address arithmetic per load, load -> wait -> MFMA per
// k-block.  Read through an SGPR the index is uniform: scalar loop control and the requested unrolling / prefetch distance.
#ifdef __HIPCC__
#define DS_WAVE_ID(tid) __builtin_amdgcn_readfirstlane((int)(tid) >> 6)
#endif
#include "plan_types.hpp"      // ceil_div, round_up, pad_M, pad_Mw, WgradJob, RedJob (plain host code)
// largest padded inducing count: up to 1024 the LDS-resident chains, above it the GEMM-formulated passes only
#define DSDGP_MAX_MP 2048

// ------------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
typedef double d4 __attribute__((ext_vector_type(4)));
// Pointers that reach a kernel through a descriptor in MEMORY (job lists, GemmProblem, PotrfItem, LayerDev) have no known
// address space: the compiler emits flat_load / flat_store, which count on lgkmcnt as well as vmcnt — every LDS wait then also
// waits for outstanding global traffic.  Hot loops cast such pointers to the global (1) or LDS (3) address space.
typedef const double __attribute__((address_space(1)))* gcptr;
typedef double __attribute__((address_space(1)))* gptr;
typedef double __attribute__((address_space(3)))* lptr;

// Index of the segment a workgroup belongs to in a launch built from a device-resident list (jobs / problems with ascending start
// offsets): bisection, log2(n) dependent (scalar) loads.  The linear walk every grouped kernel started with costs one dependent L2 round
// trip per list entry — up to ~35 of them (the split-K reduction of a three-layer model) in front of a 20 us launch's last workgroups.
#define DS_FIND_SEGMENT(idx, list, n, field, key)            \
  do {                                                       \
    int lo__ = 0, hi__ = (n)-1;                              \
    while (lo__ < hi__) {                                    \
      const int mid__ = (lo__ + hi__ + 1) >> 1;              \
      if ((key) >= (list)[mid__].field) lo__ = mid__;        \
      else hi__ = mid__ - 1;                                 \
    }                                                        \
    idx = lo__;                                              \
  } while (0)

// v_mfma_f64_16x16x4_f64: D(16x16) += A(16x4) * B(4x16), wave64.
//   lane l: g = l>>4, c = l&15.   A operand = A[i=c][k=g];  B operand = B[k=g][j=c];
//   D reg t (0..3) = D[row = g + 4t][col = c].
// Note the D layout of a 16x16 block *is* the B-operand layout of four consecutive k-steps (k = g + 4t), which is
// what lets the layer chain feed one GEMM's result straight into the next without touching LDS.
__device__ __forceinline__ d4 mfma_f64(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// Cross-lane sums WITHOUT the LDS: __shfl_xor compiles to ds_bpermute_b32 pairs (an LDS round trip of 100-200 cycles per step when
// 32 waves share the CU); the per-input-dimension reductions at the end of the backward chain were six such dependent steps per
// dimension and took 23 K of the 61 K clocks of a D_out = 1 workgroup (DSDGP_BWD_TIMING, profiles/r02_chain_phases.txt, before/after in DESIGN.md 5.1).
// gfx950 has v_permlane16_swap / v_permlane32_swap (exchange odd/even 16-lane rows, upper/lower 32 lanes) and the gfx9 DPP row
// shifts / row broadcasts, all plain VALU instructions.
//
// sum over the four 16-lane groups (same c): afterwards every lane holds the total for its column c.
__device__ __forceinline__ double sum_groups(double x) {
  const unsigned lo = __double2loint(x), hi = __double2hiint(x);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);     // {this row | its neighbour row} in either order
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double y = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
  const unsigned lo2 = __double2loint(y), hi2 = __double2hiint(y);
  const auto c = __builtin_amdgcn_permlane32_swap(lo2, lo2, false, false);
  const auto d = __builtin_amdgcn_permlane32_swap(hi2, hi2, false, false);
  return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_or_zero(double x) {      // the DPP-moved value; lanes without a source (or masked off) read 0
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROWMASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// full 64-lane sum, returned in every lane (inclusive scan by row_shr 1/2/4/8, row_bcast 15/31, then lane 63 read back)
__device__ __forceinline__ double sum_wave(double x) {
  x += dpp_or_zero<0x111, 0xf>(x);
  x += dpp_or_zero<0x112, 0xf>(x);
  x += dpp_or_zero<0x114, 0xf>(x);
  x += dpp_or_zero<0x118, 0xf>(x);
  x += dpp_or_zero<0x142, 0xa>(x);
  x += dpp_or_zero<0x143, 0xc>(x);
  const unsigned lo = __builtin_amdgcn_readlane((int)__double2loint(x), 63);
  const unsigned hi = __builtin_amdgcn_readlane((int)__double2hiint(x), 63);
  return __hiloint2double(hi, lo);
}

// sum over a workgroup of T threads (a power of two) of x, every thread receives it: thread t's value enters at leaf t of a fixed tree
// over red[T] (LDS), so the same values give the same bits.  The leading barrier lets calls follow each other on one array.
template <int T>
__device__ __forceinline__ double block_sum(double x, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = x;
  __syncthreads();
  for (int h = T / 2; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// broadcast of lane `L` (compile-time constant) of a double through two v_readlane_b32 (far cheaper than the
// ds_bpermute pair behind __shfl)
template <int L>
__device__ __forceinline__ double bcast_lane(double x) {
  const unsigned lo = __builtin_amdgcn_readlane((int)__double2loint(x), L);
  const unsigned hi = __builtin_amdgcn_readlane((int)__double2hiint(x), L);
  return __hiloint2double((int)hi, (int)lo);
}

// hyper-parameter block layout (device doubles) produced by k_prep for every layer:
//   hyp[0]=variance hyp[1]=white_variance hyp[2]=kdiag (=variance+white) hyp[3]=sigmoid(raw var) hyp[4]=sigmoid(raw white)
//   hyp[8 + j]            = 1/lengthscale_j                   (j < D_in)
//   hyp[8 + D_in + j]     = sigmoid(raw lengthscale_j)        (chain rule of the softplus transform)
#define HYP_VAR 0
#define HYP_WVAR 1
#define HYP_KDIAG 2
#define HYP_DVAR 3
#define HYP_DWVAR 4
#define HYP_ILS 8

// stationary kernel value and d k / d r2 from the scaled squared distance r2 (variance included).
//   RBF      [UPSTREAM]: k = s2 exp(-r2/2)
//   Matern52 [UPSTREAM]: r = sqrt(r2 + 1e-12); k = s2 (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)
template <int KIND>
__device__ __forceinline__ double kern_val(double r2, double s2) {
  if (KIND == DSDGP_KERN_RBF) return s2 * exp(-0.5 * r2);
  const double s5 = 2.23606797749978969641;
  double r = sqrt(r2 + 1e-12);
  return s2 * (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * exp(-s5 * r);
}
template <int KIND>
__device__ __forceinline__ void kern_val_grad(double r2, double s2, double& k, double& dk) {
  if (KIND == DSDGP_KERN_RBF) {
    k = s2 * exp(-0.5 * r2);
    dk = -0.5 * k;
    return;
  }
  const double s5 = 2.23606797749978969641;
  double r = sqrt(r2 + 1e-12);
  double e = s2 * exp(-s5 * r);
  k = (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * e;
  dk = -(5.0 / 6.0) * (1.0 + s5 * r) * e;
}
__device__ __forceinline__ double kern_val_rt(int kind, double r2, double s2) {
  return kind == DSDGP_KERN_RBF ? kern_val<DSDGP_KERN_RBF>(r2, s2) : kern_val<DSDGP_KERN_MATERN52>(r2, s2);
}
#endif
