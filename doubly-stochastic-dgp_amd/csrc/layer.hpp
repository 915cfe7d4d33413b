// SVGP_Layer hot path on gfx950: argument blocks of the chain kernels and of the split-K weight-gradient products.
#pragma once
#include "common.hpp"
#include "chain_policy.hpp"   // the size rules of these launches (XCH, sm_*, chain_d_split, layer_last_fusable, ...): plain host code

// SVGP_Layer.conditional_ND + reparameterize (layers.py:178-219, utils.py:40-41), fused.
struct LayerFwdArgs {
  const double* X;   // (Rin x D_in) row-major inputs (for layer 0: the N minibatch rows, shared by all S samples)
  int64_t Rin;
  int32_t rep;       // S for layer 0 (tf.tile of dgp.py:63 is never materialised), 1 otherwise
  int32_t D_in, D_out, M;
  const double* Zp;     // (Mp x D_in), rows >= M zero
  const double* Zs;     // (Mp x D_in)  Z / lengthscale (split-M kernels read it through L1/L2 instead of staging it in LDS)
  const double* hyp;    // see common.hpp HYP_*
  const double* LinvT;  // (Mp x Mp)  Lu^{-T}
  const double* Linv;   // (Mp x Mp)  Lu^{-1}
  const double* Tp;     // (D_out x Mp x Mp) lower-triangular q_sqrt, zero padded
  const double* TpT;    // (D_out x Mp x Mp) its transpose (split-M kernels read every weight as rows [i][k])
  const double* qmu;    // (Mp x D_out)
  int32_t qmu_ld;       // row stride of qmu (0: D_out)
  int32_t mean_kind;
  const double* mean_A; // (D_in x D_out) of the Linear mean function
  const double* mean_b; // (D_out) bias of the Linear mean function or NULL
  const double* z;      // N(0,1) draws, element (s,i,d) at z[s*zs_s + i*zs_n + d*zs_d]; NULL -> F not produced
  int64_t zs_s, zs_n, zs_d;
  int64_t n_inner;      // minibatch rows per sample: output row o = s*n_inner + i
  double jitter;
  double* F;            // (rep*Rin x D_out) samples or NULL
  double* mean;         // (rep*Rin x D_out) or NULL
  double* var;          // (rep*Rin x D_out) or NULL
  double* Asave;        // (Mp x ldA): A = Ku^{-1} Kuf (white: Lu^{-1} Kuf), kept for the backward pass, or NULL
  double* Csave;        // [row block][D_out][Mp slots][16 rows]: c_d = q_sqrt_d^T a of every output in LDS slot order, kept for the
                        // backward pass (split-M kernels), or NULL
  int64_t ldA;
  int32_t d_split;      // split-M kernels: gridDim.y workgroups share a row block, each taking D_out/d_split outputs
  double* XT1;          // split-M kernels, training: (DinP16 x ldA) [X^T ; 1] for the Z-gradient product, or NULL
  unsigned long long* phase_clk;   // debug aid (DSDGP_FWD_TIMING): [workgroup][8] s_memrealtime (100 MHz) stamps of the forward chain's phases, or NULL
  // last layer of a training step with the Gaussian likelihood: [UPSTREAM] Gaussian.variational_expectations (dgp.py:89-90) and its
  // adjoints in this chain's epilogue (k_lik_elbo<LIKF_GAUSS>'s job: one launch less between the forward and the reverse pass).  lik_Y NULL: off.
  const double* lik_Y;             // (n_inner x D_out) targets
  const double* lik_const;         // [0] = likelihood variance
  double lik_w;                    // data_scale / S
  double* lik_part;                // [workgroup][2]: sum of the variational expectations, sum of d / d variance
  double *lik_MB, *lik_VB;         // (D_out x lik_ld) transposed adjoints w.r.t. mean / var of this layer (the backward chain reads them)
  int64_t lik_ld;
};

struct LayerBwdArgs {
  const double* X;
  int64_t Rin;
  int32_t D_in, D_out, M, DP4;
  const double* Zp;
  const double* Zs;     // (Mp x D_in)  Z / lengthscale
  const double* hyp;
  const double* Kinv;   // (Mp x Mp)
  const double* Linv;   // (Mp x Mp)   (white path)
  const double* LinvT;  // (Mp x Mp)   (white path, split-M kernels)
  const double* Sd;     // (D_out x Mp x Mp)  q_sqrt q_sqrt^T
  const double* qmu4;   // (Mp x DP4)
  const double* Asave;
  const double* Csave;  // [row block][D_out][Mp][16] from the forward chain: abar += q_sqrt_d (2 vbar_d c_d) — a triangular product — replaces
                        // the dense 2 vbar_d S_d a (split-M kernels; NULL selects the S_d form)
  const double* Tp;     // (D_out x Mp x Mp) q_sqrt, and its transpose (Csave form)
  const double* TpT;
  int64_t ldA;
  // Pad columns [Rin, ldA) of the row-major (.. x ldA) buffers.  ldA = round_up(Rin, 16) is set per call, so on a reused model the pad
  // of a small call lies on the data of an earlier, larger one: nothing is zeroed between calls, every producer writes its own pad on
  // every call (tests/test_gpu_model_reuse.py holds a reused model to the bits of a fresh one):
  //   Asave     the forward chain stores 0 for r >= Rin (k_layer_fwd_sm's A store, the fused last-layer launch; the GEMM pass through
  //             the zero pad of k_kuf's K)
  //   XT1       [X^T;1]: 0 for r >= Rin — the forward chain's XT1 store, k_xt1 (GEMM pass), k_adj_prep
  //   VB, MB    whoever produces the adjoints: the next layer's backward chain (MBp / VBp: zeros for Rin <= row < ldA), the adjoint
  //             prologue of this chain (MBw / VBw, same), k_adj_prep (every r < ld, 0 where r >= Rin or d >= D_out), the likelihood
  //             epilogue of the last forward chain (lik_MB / lik_VB) and k_lik_elbo (MBt / VBt)
  //   GW        this chain, all ldA columns: 0 where r >= Rin or m >= M
  //   E         this chain, all ldA columns; the pad holds whatever the chain computed for the clamped rows — its only consumer, the
  //             product E A^T, meets Asave's zero pad there
  // Most consumers do not rely on one pad alone: the chain selects vbar = 0 for r >= ldA only, but the products over the row index
  // (A diag(vbar_d) A^T, A mbar^T, E A^T) have Asave's zero pad as an operand, GW [X^T;1]^T has two zero pads, and the
  // hyper-parameter partial sums are masked with r < Rin.  The split-K partials are another matter: ensure_plan zeroes part_big and the
  // tickets when the shape changes, because diagonal tiles fill only their first ns_diag slots (dropping that reset fails the test).
  const double* VB;     // (D_out.. x ldA)  d loss / d var, transposed, zero beyond Rin
  const double* MB;     // (>=DP4 x ldA)    d loss / d mean, transposed, zero padded
  double* E;            // (Mp x ldA)  out: so that d loss/d Ku (data) = -sym(E A^T)
  double* GW;           // (Mp x ldA)  out: Kuf-bar * dk/dr2
  double* dX;           // (Rin x D_in) out or NULL
  int32_t mean_kind;
  const double* mean_A;
  double* hyp_part;     // [nwaves][D_in + 2]: sum kbar*k, sum vbar, lengthscale partials
  // split-M kernels: when the PREVIOUS layer is an inner layer (one output row per input row) its transposed upstream
  // adjoints are written here directly (k_adj_prep's job): MBp[d][r] = dX[r][prop+d], VBp[d][r] = dX * z / (2 sqrt(var+jitter))
  double* MBp;          // (>= Dp x ldA) or NULL (then dX is written instead)
  double* VBp;
  const double* zp;     // the previous layer's N(0,1) draws, element (row, d) at zp[(row / n_inner) * zp_s + (row % n_inner) * zp_n + d * zp_d]
  int64_t zp_s, zp_n, zp_d, n_inner;
  const double* varp;   // the previous layer's variances (Rin x Dp)
  int32_t Dp, prop;     // previous layer's D_out, input_prop_dim
  double jitter;
  unsigned long long* phase_clk;   // debug aid (DSDGP_BWD_TIMING): [workgroup][8] s_memrealtime (100 MHz) stamps of the backward chain's phases, or NULL
  // split-M kernels, small launches: gridDim.y = d_split workgroups share a row block, each takes D_out / d_split outputs of the d-loop
  // and leaves its partial abar tile (+ its share of sum_d vbar_d) in `part` ([row block][d_split][Mp * 16 + 16]); the workgroup that
  // arrives last (ticket from part_cnt[row block], reset by it) adds the partials in split order — a fixed order, whoever is
  // last — and runs the rest of the chain
  int32_t d_split;
  double* part;
  int* part_cnt;
  // a layer with `up_rep` output rows per input row (the first layer: S samples share mean / var) gets its transposed upstream adjoints
  // from the adjoint of the next layer's input right here, in the chain's prologue (k_adj_prep's job, one launch less on the
  // critical path):  MB[d][r] = sum_s dF[s Rin + r][off + d],  VB[d][r] = sum_s dF[..] z[..] / (2 sqrt(var[r][d] + jitter)); written
  // to MB / VB (the weight-gradient products read them too) by the workgroup that owns the row block.  NULL: MB / VB are ready.
  const double* up_dF;
  int32_t up_rep, up_ld, up_off;
  const double* up_z;          // this layer's draws, element (row, d) at up_z[(row / n_inner) * up_zs + (row % n_inner) * up_zn + d * up_zd]
  int64_t up_zs, up_zn, up_zd, up_n_inner;
  const double* up_var;        // this layer's variances (Rin x D_out)
  double up_jitter;
  double *MBw, *VBw;           // = MB / VB, writable
};

// jobs_dev: device copy (WgradJob: plan_types.hpp) of `njobs` jobs with task_start filled (64 x 64 tiles, one workgroup per (job, split, tile) task; grouped
// jobs: one workgroup per (split, 32 x 32 tile) task of the group's outputs)
int wgrad_launch(dsdgp_ctx* ctx, const WgradJob* jobs_dev, int njobs, int total_tasks, int nsplit, int64_t ld, int64_t Rp,
                 hipStream_t stream = nullptr);
// chain kernels (layer_sm.hip): the NW waves of a workgroup cooperate on one block of 16 rows
int layer_fwd_sm_launch(dsdgp_ctx* ctx, const LayerFwdArgs& a, int Mp, int kern_kind, int white);
int layer_bwd_sm_launch(dsdgp_ctx* ctx, const LayerBwdArgs& a, int Mp, int kern_kind, int white);
// the last layer of a training step as one launch (layer_last.hip): forward chain + Gaussian likelihood + reverse mode of the same row
// block.  Its scope is layer_last_fusable (chain_policy.hpp), decided at forward time; the launch asserts it on its two argument blocks.
int layer_last_launch(dsdgp_ctx* ctx, const LayerFwdArgs& a, const LayerBwdArgs& b, int Mp, int kern_kind, int hyp_rows);

// ------------------------------------------------------------------------------------------------------
// GEMM-formulated layer passes for LARGE inducing counts (layer_gemm.hip; Mp >= 512 by default).
// The fused chains keep one block of 16 data rows per workgroup, so every weight element fetched from L2 / Infinity Cache feeds 16
// columns of one MFMA — at Mp >= 512 the weights of a layer (2 + D_out triangular M x M matrices, 10 - 40 MB) no longer sit in L1 / L2
// and the chains run at 0.16 - 0.31 of the fp64 MFMA peak (profiles/r03_kernel_stats_cfg{4,5}.md).  Here each of the layer's products
// is ONE LDS-tiled MFMA GEMM over the whole row range (128 x 128 output tiles: every weight and every activation element is used 128
// times per fetch), with the per-row reductions (|a1|^2, |c_d|^2) taken in the GEMM epilogue; the intermediates (Kuf, a1, a, c_d:
// Mp x R doubles each, 51 MB at config 5) live in HBM / Infinity Cache between the launches.
// Same argument blocks and same outputs as the chains (A, C, mean / var / F, E, GW, hyp_part, dX / MBp / VBp), so the
// weight-gradient products, the assembly and the optimiser are untouched.  C (c_d for the backward pass) is laid out [d][Mp][ldA].
// ------------------------------------------------------------------------------------------------------
struct GemmLayerWs {
  double* T1;        // (Mp_max x ld_max)  forward: Kuf            backward: Ku^-1 abar
  double* T2;        // (Mp_max x ld_max)  forward: a1 = Lu^-1 Kuf backward: abar
  double* Pb;        // (GL_MAX_GROUPS + 1) x (Mp_max x ld_max): partial abar of the d-groups + the mean part
  double* colsq;     // (1 + D_out_max) x tiles_m_max x ld_max: per-tile-row column sums of squares (|a1|^2, |c_d|^2)
  double* MUT;       // (DP16_max x ld_max)  q_mu^T a
  double* qmuT;      // (DP16_max x Mp_max)  q_mu^T, zero padded
  double* ZZ;        // (Mp_max x nzz_max)   [Z/l | (Z/l)^2 | 1]
  double* OUTt;      // (nzz_max x ld_max)   ZZ^T GW
  double* svar;      // per block of the element-wise backward kernel: sum kbar k
  int64_t pb_doubles; // capacity of Pb
};
#define GL_MAX_GROUPS 4
int layer_gemm_hyp_parts(int64_t ld, int Mp);
int layer_fwd_gemm_launch(dsdgp_ctx* ctx, const LayerFwdArgs& a, int Mp, int kern_kind, int white, const GemmLayerWs& ws);
int layer_bwd_gemm_launch(dsdgp_ctx* ctx, const LayerBwdArgs& b, int Mp, int kern_kind, int white, const GemmLayerWs& ws);
