/*
 * dsdgp.h — C-ABI of the MI355X-native doubly-stochastic DGP hot path (libdsdgp.so, gfx950).
 *
 * The reference (UCL-SML/Doubly-Stochastic-DGP) has NO FFI / plugin interface: its hot path is reached only
 * through Python classes that compose GPflow/TF ops.  Each entry point below therefore cites the reference
 * *call site* (file:line under /root/reference) whose TF/GPflow op sequence it replaces.  A maintainer binds
 * these with ctypes; the shipped host mirror lives in
 * doubly-stochastic-dgp_amd/doubly_stochastic_dgp/.
 *
 * Conventions
 *   - every function returns int: 0 = DSDGP_OK, <0 = dsdgp_status; dsdgp_last_error() gives a thread-local
 *     message (the reference surfaces errors as Python exceptions from session.run, e.g. "Cholesky
 *     decomposition was not successful" — the host mirror re-raises DSDGP_ERR_NOT_SPD the same way).
 *   - all data pointers are DEVICE pointers to row-major float64 unless marked "host"; the caller owns every
 *     buffer (including workspaces); the library never frees caller memory and keeps model-bound pointers only
 *     until dsdgp_model_destroy.
 *   - work is enqueued asynchronously on the ctx stream; dsdgp_sync() waits for it.
 *   - all arithmetic is float64 (settings.float_type, layers.py:68).
 */
#ifndef DSDGP_H
#define DSDGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsdgp_ctx dsdgp_ctx;
typedef struct dsdgp_model dsdgp_model;

typedef enum {
  DSDGP_OK = 0,
  DSDGP_ERR_BAD_ARG = -1,
  DSDGP_ERR_NOT_SPD = -2,      /* tf.cholesky failure, layers.py:172 */
  DSDGP_ERR_HIP = -3,
  DSDGP_ERR_UNSUPPORTED = -4,
  DSDGP_ERR_WORKSPACE = -5,
  DSDGP_ERR_RCCL = -6          /* dsdgp_allreduce: RCCL missing or a collective failed */
} dsdgp_status;

enum { DSDGP_KERN_RBF = 0, DSDGP_KERN_MATERN52 = 1 };            /* [UPSTREAM] gpflow.kernels */
enum { DSDGP_MEAN_ZERO = 0, DSDGP_MEAN_IDENTITY = 1, DSDGP_MEAN_LINEAR = 2 }; /* layer_initializations.py:30-42,51 */
enum { DSDGP_LIK_GAUSSIAN = 0, DSDGP_LIK_MULTICLASS = 1, DSDGP_LIK_BERNOULLI = 2,     /* dgp.py:57, utils.py:54-93,
                                                                                       * tests/test_dgp.py:48-54 */
       /* further likelihoods utils.py:54-121 can wrap ([UPSTREAM] gpflow 1.1.1 likelihoods.py), exp links / StudentT: */
       DSDGP_LIK_POISSON = 3, DSDGP_LIK_EXPONENTIAL = 4, DSDGP_LIK_STUDENT_T = 5, DSDGP_LIK_GAMMA = 6, DSDGP_LIK_BETA = 7 };

#define DSDGP_MAX_LAYERS 16

/* ---- context ---------------------------------------------------------------------------------------- */
int dsdgp_version(void);
/* sizeof(dsdgp_layer_desc) / sizeof(dsdgp_model_desc) as compiled: a binding checks its struct mirrors against these. */
int dsdgp_sizeof_layer_desc(void);
int dsdgp_sizeof_model_desc(void);
const char* dsdgp_last_error(void);
/* stream: a hipStream_t (as void*) to enqueue on, or NULL for a library-owned stream. */
int dsdgp_ctx_create(dsdgp_ctx** out, int device, void* stream);
int dsdgp_ctx_destroy(dsdgp_ctx* ctx);
int dsdgp_sync(dsdgp_ctx* ctx);
/* HIP-event timing of the most recent launch of a named kernel class on the ctx stream (bench.py roofline):
 * enable, run, then read the accumulated milliseconds and launch count. name in
 * {"layer_fwd","layer_bwd","wgrad","gram","potrf","gemm","evaluate","calibration","pca_gram","pca_eig","psi","psi2","gram_grad","pathwise"}. */
int dsdgp_prof_enable(dsdgp_ctx* ctx, int on);
int dsdgp_prof_read(dsdgp_ctx* ctx, const char* name, double* total_ms, int64_t* launches, int reset);
/* Kernel launches this library has enqueued in this process so far (all contexts; memsets / copies not counted): the difference
 * around a loop of steps is that loop's launches per step (bench.py `launches_per_step`).  No reference counterpart: measurement aid. */
int64_t dsdgp_launch_count(void);

/* ---- primitives (north_star: Gram assembly, blocked Cholesky, trsm) ----------------------------------- */
/* Kernel hyper-parameters, host side.  lengthscales: host pointer to 1 (ard=0) or input_dim (ard=1) values. */
typedef struct {
  int32_t kind;            /* DSDGP_KERN_* */
  int32_t input_dim;
  int32_t ard;
  int32_t has_white;       /* k + White(white_variance): only K(X) and Kdiag see it */
  double variance;
  double white_variance;
  const double* lengthscales; /* host */
} dsdgp_kernel;

/* K1/K3 — feature.Kuu(kern, jitter) / feature.Kuf(kern, X) (layers.py:171,184 -> [UPSTREAM] kern.K):
 *   X2 == NULL : out[n,n]  = k(X,X) + (white_variance + jitter) I          (symmetric)
 *   else       : out[n,n2] = k(X,X2)                                       (White contributes 0)   */
int dsdgp_gram(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, const double* X2, int64_t n2,
               double jitter, double* out, int64_t ld_out);

/* K2 — tf.cholesky (layers.py:172): in-place lower Cholesky of `batch` n x n SPD matrices (upper part zeroed).
 * info (host, may be NULL): 0 ok, i>0 = first non-positive pivot (1-based) in some batch entry.
 * Blocked right-looking factorisation; the trailing update is an fp64-MFMA syrk/gemm. */
int dsdgp_potrf(dsdgp_ctx* ctx, int batch, int n, double* A, int64_t lda, int64_t stride, int* info);

/* K4 — tf.matrix_triangular_solve(L, B, lower=True) and its transposed form (layers.py:186,188):
 *   trans=0: B <- L^{-1} B ;  trans=1: B <- L^{-T} B.   L: n x n lower (only the lower triangle is read), B: n x nrhs, in place.
 * Blocked: 16 x 16 diagonal-block inverses with one refinement step per block (componentwise backward error at the level of a
 * substitution's), 128-row panels solved one wave per 16 right-hand-side columns (MFMA products chained in registers), MFMA GEMM
 * updates of the rows below / above a panel.  n^2 nrhs flops; any n, any nrhs; asynchronous. */
int dsdgp_trsm(dsdgp_ctx* ctx, int trans, int n, int64_t nrhs, const double* L, int64_t ldl, double* B, int64_t ldb);
/* The batched form of layers.py:239, tf.matrix_triangular_solve(self.Lu_tiled, self.q_sqrt): `batch` right-hand-side matrices
 * strideB doubles apart, their L matrices strideL apart — strideL = 0: ONE L shared by the batch (the reference tiles Lu D_out
 * times, layers.py:173; nothing is tiled here). */
int dsdgp_trsm_batched(dsdgp_ctx* ctx, int trans, int n, int64_t nrhs, int batch, const double* L, int64_t ldl, int64_t strideL,
                       double* B, int64_t ldb, int64_t strideB);

/* plain fp64-MFMA GEMM used by the M x M algebra: C = alpha op(A) op(B) + beta C (row-major). */
int dsdgp_gemm(dsdgp_ctx* ctx, int transA, int transB, int m, int n, int k, double alpha, const double* A,
               int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);

/* ---- model: DGP_Base / SVGP_Layer (dgp.py:42-126, layers.py:122-246) ----------------------------------- */
typedef struct {
  int32_t M, D_in, D_out;          /* SVGP_Layer.__init__ layers.py:123-165 */
  int32_t kern_kind, ard, has_white;
  int32_t mean_kind;               /* DSDGP_MEAN_* */
  int32_t trainable_Z, trainable_q_mu, trainable_q_sqrt, trainable_kvar, trainable_kls, trainable_wvar;
  int32_t input_prop_dim;          /* Layer(input_prop_dim) layers.py:36-50,105-117: the next layer sees [X[:, :p] | samples] */
  int32_t trainable_mean_A, trainable_mean_b;   /* only meaningful when the corresponding off_mean_* >= 0 */
  int32_t kvar_identity;           /* 1: theta[off_kvar] IS the kernel variance (a Parameter without transform — the reference's own
                                      tests build such a kernel to reach variance 1e-24, tests/test_dgp.py:79-85); 0: softplus + 1e-6 */
  int32_t reserved0;
  const double* mean_A;            /* device, (D_in x D_out) for DSDGP_MEAN_LINEAR when fixed (layer_initializations.py:41-42);
                                      ignored when off_mean_A >= 0 */
  /* offsets (in doubles) into the flat unconstrained parameter vector theta: */
  int64_t off_Z;                   /* (M, D_in)                       feature.Z           layers.py:153 */
  int64_t off_q_mu;                /* (M, D_out)                      layers.py:146-147 */
  int64_t off_q_sqrt;              /* (D_out, M, M) dense; tril part is the free variable  layers.py:149-151 */
  int64_t off_kvar;                /* scalar, softplus^-1(variance)   [UPSTREAM] transforms.positive (the variance itself if kvar_identity) */
  int64_t off_kls;                 /* 1 or D_in values, softplus^-1(lengthscales) */
  int64_t off_wvar;                /* scalar (if has_white) */
  /* [UPSTREAM] mean_functions.Linear(A, b) as a free parameter (a user-supplied final mean function, dgp.py:187): */
  int64_t off_mean_A;              /* (D_in, D_out) row-major inside theta, or -1: use the fixed mean_A pointer */
  int64_t off_mean_b;              /* (D_out) inside theta, or -1: no bias */
} dsdgp_layer_desc;

typedef struct {
  int32_t L;
  int32_t white;                   /* DGP(..., white=False) dgp.py:187 */
  int32_t lik_kind;
  int32_t num_classes;
  int32_t trainable_lik_var;
  int32_t reserved;
  double jitter;                   /* settings.jitter, layers.py:171, utils.py:41 */
  double lik_aux;                  /* the likelihood's constant: Poisson.binsize, StudentT.deg_free (else ignored) */
  int64_t off_lik_var;             /* scalar, softplus^-1 of the likelihood's positive parameter: Gaussian.variance, StudentT.scale,
                                      Gamma.shape, Beta.scale */
  int64_t n_theta;
  dsdgp_layer_desc layers[DSDGP_MAX_LAYERS];
} dsdgp_model_desc;

/* Workspace needed for minibatches of up to n_max rows and s_max samples. */
int dsdgp_model_workspace_bytes(const dsdgp_model_desc* desc, int64_t n_max, int32_t s_max, int64_t* bytes);
/* theta/grad/adam_m/adam_v: device, n_theta doubles each, 16-byte aligned (DSDGP_ERR_BAD_ARG otherwise: the optimiser reads them as
 * pairs); grad/adam_* may be NULL for predict-only models.  workspace: 256-byte aligned. */
int dsdgp_model_create(dsdgp_ctx* ctx, const dsdgp_model_desc* desc, int64_t n_max, int32_t s_max, double* theta,
                       double* grad, double* adam_m, double* adam_v, void* workspace, int64_t workspace_bytes,
                       dsdgp_model** out);
int dsdgp_model_destroy(dsdgp_model* m);

/* build_cholesky_if_needed for every layer (layers.py:167-175): Ku, Lu (+ Lu^-1, Ku^-1) from the current theta.
 * Must precede propagate / layer calls after theta changed; dsdgp_model_elbo calls it itself.
 * info (host, may be NULL) is filled after an implicit sync with the Cholesky status. */
int dsdgp_model_prepare(dsdgp_model* m, int* info);

/* DGP_Base.propagate (dgp.py:61-76) with full_cov=False.
 *   X (n x D_in0) device. zs: host array of L device pointers (or NULL entries / NULL array): explicit N(0,1) draws
 *   for layer l; element (s,i,d) is read at zs[l][s*zstride[3l] + i*zstride[3l+1] + d*zstride[3l+2]] (strides in
 *   doubles, 0 = broadcast; dgp.py:62,68 "zs" injection).  NULL -> on-device Philox draws from `seed`.
 *   Fs/Fmeans/Fvars: host arrays of L device pointers ((S*n) x D_out_l each, row (s*n+i)) or NULL / NULL entries. */
int dsdgp_model_propagate(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs,
                          const int64_t* zstride, uint64_t seed, double* const* Fs, double* const* Fmeans,
                          double* const* Fvars);

/* DGP_Base._build_likelihood (dgp.py:92-98) on an explicit minibatch, optionally with the reverse-mode gradient of
 * loss = -(data_scale * sum_n E_log_p_Y - kl_weight * sum_l KL_l) w.r.t. theta written to `grad`
 * (stands in for tf.gradients [UPSTREAM]).  data_scale = num_data / n_global (dgp.py:96-97); kl_weight = 1, or
 * 1/world_size when the row-sharded data-parallel all-reduce sums ranks.
 * out (device, 4 doubles): [elbo_local, data_term (scaled), kl_weight * KL_sum, potrf_info (0 ok, else 1-based failing pivot)].
 * Every entry but the last sums over data-parallel ranks to the single-process value; potrf_info is identical on all ranks
 * (parameters are replicated), i.e. the sum is world_size * pivot. */
int dsdgp_model_elbo(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S,
                     const double* const* zs, const int64_t* zstride, uint64_t seed, double data_scale,
                     double kl_weight, int with_grad, double* out);

/* Vector-Jacobian product of the layers, in two calls: for a scalar J of the LAST layer's mean and variance that somebody else
 * evaluates (model_zoo.py:52-57: the collapsed bound of DGP_Collapsed reads the inner layers' last mean and variance — the reference
 * lets TensorFlow differentiate through them), the gradient of J - kl_weight * sum_l KL_l with respect to theta.
 *
 * dsdgp_model_forward_saved: the forward pass of a gradient evaluation (what dsdgp_model_elbo(with_grad = 1) does ahead of its
 *   likelihood: draws, parameter products, the layers' chains keeping what the reverse pass reads) without a likelihood and without a
 *   sample of the last layer.  X, n, S, zs, zstride, seed as for dsdgp_model_propagate (zs[L-1] is not read).  mean_out / var_out:
 *   device, (S*n) x D_out of the last layer, row (s*n+i); either may be NULL (the values stay in the workspace).
 *   The saved state is the model's until its next call of any kind but dsdgp_model_backward_adjoints: another evaluation
 *   (propagate, elbo, training step, the mixture entries, layer_conditional*), dsdgp_model_theta_changed, an optimiser step or
 *   dsdgp_model_prepare drops it.
 * dsdgp_model_backward_adjoints: dmean / dvar (device, the layout of mean_out / var_out) are dJ/dmean and dJ/dvar.  Runs the reverse
 *   pass of the saved forward pass and leaves the gradient of  loss = -(J - kl_weight * sum_l KL_l)  in `grad`: layout and sign as
 *   dsdgp_model_elbo(with_grad = 1) leaves them, a FULL gradient (dsdgp_model_adam_step accepts it).  The likelihood takes no part:
 *   its parameter's entry of `grad` is +0.0.  out (device, 4 doubles): [-kl_weight * KL_sum, 0, kl_weight * KL_sum, potrf_info].
 *   The saved state is consumed: one reverse pass per forward pass.
 * DSDGP_ERR_BAD_ARG: no saved forward pass is the model's last evaluation; the reverse pass is restricted
 * (dsdgp_model_set_grad_first_layer / _q_only).  DSDGP_ERR_UNSUPPORTED: a bucket callback or quadrature sample weights are set.  A
 * refused dsdgp_model_backward_adjoints writes nothing. */
int dsdgp_model_forward_saved(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs, const int64_t* zstride,
                              uint64_t seed, double* mean_out, double* var_out);
int dsdgp_model_backward_adjoints(dsdgp_model* m, const double* dmean, const double* dvar, double kl_weight, double* out);

/* DGP_Quad (dgp.py:129-166): replace the Monte-Carlo mean over the S propagated samples of dsdgp_model_elbo by the
 * weighted sum  sum_s w[s] (.)  (Gauss-Hermite weights, summing to one).  w: device, S doubles, borrowed until cleared;
 * NULL restores the mean.  dsdgp_model_elbo then requires its S argument to equal this S. */
int dsdgp_model_set_sample_weights(dsdgp_model* m, const double* w, int32_t S);

/* [UPSTREAM] tf.train.AdamOptimizer step on theta using grad (t counts from 1). Non-trainable entries are skipped. */
int dsdgp_model_adam_step(dsdgp_model* m, double lr, double beta1, double beta2, double eps, int64_t t);

/* One optimiser step of -ELBO in ONE call — `session.run(opt_op)` of demos/demo_regression_UCI.ipynb:324 with
 * opt_op = AdamOptimizer(lr).minimize(model): dsdgp_model_elbo(with_grad = 1) followed by the Adam update (t counts from 1), the
 * update applied by the last launch of the reverse pass instead of a launch of its own.  Same arguments and `out` as
 * dsdgp_model_elbo; `grad` holds the gradient the update used.  Single-process training only: a data-parallel step needs the
 * all-reduce between the two halves (dsdgp_model_elbo, dsdgp_allreduce, dsdgp_model_adam_step).  DSDGP_ERR_BAD_ARG while
 * dsdgp_model_set_grad_first_layer / dsdgp_model_set_grad_q_only restrict the reverse pass (the caller lifts the restriction first:
 * the step does not do it on the caller's behalf). */
int dsdgp_model_train_step(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                           const int64_t* zstride, uint64_t seed, double data_scale, double kl_weight, double lr, double beta1,
                           double beta2, double eps, int64_t t, double* out);

/* dsdgp_model_train_step on the minibatch rows idx[idx_offset .. idx_offset + n) of the resident data X_all (rows x D_in of the first
 * layer) / Y_all (rows x D_Y): the two Minibatch iterators of dgp.py:51-52 and the optimiser step in one call; the gather runs inside
 * the step's first launch.  idx: device int64.  Fresh N(0,1) draws (Philox, `seed`); no explicit zs. */
int dsdgp_model_train_step_minibatch(dsdgp_model* m, const double* X_all, const double* Y_all, const int64_t* idx, int64_t idx_offset,
                                     int64_t n, int32_t S, uint64_t seed, double data_scale, double kl_weight, double lr, double beta1,
                                     double beta2, double eps, int64_t t, double* out);

/* [UPSTREAM] gpflow.training.NatGradOptimizer(gamma) step on layer l's (q_mu, q_sqrt), using the loss gradient left in
 * `grad` by the last dsdgp_model_elbo(with_grad=1) (demos/demo_regression_UCI.ipynb:360-366, tests/test_collapsed.py:100):
 * per output, natural parameters theta <- theta - gamma dL/d eta, then back to (mean, Cholesky factor).
 * info (host, may be NULL): non-zero (with DSDGP_ERR_NOT_SPD) if A = S^-1 + 2 gamma dL/dS is not SPD for some output.  Such a
 * step is refused as a whole, with or without info: theta is not written ([UPSTREAM] tf.cholesky raises, no variable is assigned). */
int dsdgp_model_natgrad_step(dsdgp_model* m, int32_t l, double gamma, int* info);

/* [UPSTREAM] tf.gradients(loss, var_list) with var_list = the (q_mu, q_sqrt) of the upper layer(s), as
 * NatGradOptimizer.minimize(var_list=[[last.q_mu, last.q_sqrt]]) builds it: TensorFlow prunes the reverse pass below the
 * lowest layer in var_list.  After this call dsdgp_model_elbo(with_grad=1) runs the reverse pass for layers >= first only;
 * the gradient entries of the layers below keep their previous content (dsdgp_model_adam_step then fails with
 * DSDGP_ERR_BAD_ARG until a full gradient has been evaluated again).
 * first = 0 restores the full gradient.  Ignored (full gradient) for white=True models. */
int dsdgp_model_set_grad_first_layer(dsdgp_model* m, int32_t first);

/* [UPSTREAM] the same tf.gradients(loss, var_list) when var_list holds NOTHING BUT (q_mu, q_sqrt) pairs — what
 * NatGradOptimizer.minimize always passes (demos/demo_regression_UCI.ipynb:360-366, tests/test_collapsed.py:100): TensorFlow's reverse
 * pass then never visits Kuf / Kuu of the lowest layer in var_list (their adjoints feed Z, the kernel hyper-parameters and the layers
 * below only).  on != 0: dsdgp_model_elbo(with_grad=1) leaves complete (q_mu, q_sqrt) entries for the layers >= first
 * (dsdgp_model_set_grad_first_layer) and UNDEFINED values in their other entries.  dsdgp_model_adam_step fails with DSDGP_ERR_BAD_ARG
 * until a full gradient has been evaluated again; dsdgp_model_train_step[_minibatch] (which would evaluate its own gradient under
 * the restriction) fails with DSDGP_ERR_BAD_ARG for as long as the restriction is set: call dsdgp_model_set_grad_q_only(m, 0) and
 * dsdgp_model_set_grad_first_layer(m, 0) first.  on = 0 restores the full gradient.  Ignored for white=True models. */
int dsdgp_model_set_grad_q_only(dsdgp_model* m, int32_t on);

/* Optional contract for callers that alternate optimisers (demo_regression_UCI.ipynb:360-366: one Adam step on the hyper-parameters,
 * one natural-gradient step on the last layer).  theta is caller-owned, so every evaluation normally rebuilds Ku, its Cholesky
 * factor and the inverses (layers.py:167-175 build_cholesky_if_needed).  With tracking enabled the caller promises to report its
 * own writes to theta through dsdgp_model_theta_changed; an evaluation whose only change since the previous one came from
 * dsdgp_model_natgrad_step — which leaves Z and the kernel hyper-parameters untouched — then keeps Lu, Lu^-1 and Ku^-1 and only
 * rebuilds what depends on (q_mu, q_sqrt).  dsdgp_model_adam_step always invalidates. */
int dsdgp_model_track_theta(dsdgp_model* m, int enable);
int dsdgp_model_theta_changed(dsdgp_model* m);

/* SVGP_Layer.KL (layers.py:221-246) of layer l after dsdgp_model_prepare; out: device scalar. */
int dsdgp_model_layer_kl(dsdgp_model* m, int32_t l, double* out);

/* Read-only view of what the factorisation of layer l's Ku left behind (verification aid: nothing on the evaluation path calls it).
 * Copies the WHOLE padded Mp x Mp buffer exactly as stored — identity pad rows / columns and the halves that no kernel ever writes
 * included, no arithmetic, no clean-up — to out (host or device memory, row-major, leading dimension ld_out >= Mp; Mp is the padded
 * inducing count: 32 up to M = 32, then M rounded up to 16 / 32 / 64 / 128 for M <= 128 / 256 / 512 / above).  Prepares the model if
 * needed (dsdgp_model_prepare), waits for the parameter-side work of the side stream, and returns after the copy has completed.
 *   DSDGP_MAT_LU      Lu = chol(Ku), lower, zero above the diagonal.  Kept by white = True models only (the Cholesky adjoint reads
 *                     it); with white = False no path writes the factor back (the head launch never leaves LDS, the one-workgroup
 *                     kernels skip the write-back, the look-ahead sequence leaves its panels parked above the diagonal):
 *                     DSDGP_ERR_UNSUPPORTED rather than stale data.
 *   DSDGP_MAT_LUINV   Lu^-1, lower.  Every model, every path.
 *   DSDGP_MAT_LUINVT  Lu^-T, upper: the same numbers as DSDGP_MAT_LUINV, transposed.  Every model, every path.
 *   DSDGP_MAT_KUINV   Ku^-1 = Lu^-T Lu^-1, full symmetric matrix.  Every model, every path. */
enum { DSDGP_MAT_LU = 0, DSDGP_MAT_LUINV = 1, DSDGP_MAT_LUINVT = 2, DSDGP_MAT_KUINV = 3 };
int dsdgp_model_layer_matrix(dsdgp_model* m, int32_t l, int32_t which, double* out, int64_t ld_out);

/* SVGP_Layer.conditional_ND (layers.py:178-219, full_cov=False) of layer l on X (n x D_in_l):
 * mean, var: (n x D_out_l). */
int dsdgp_model_layer_conditional(dsdgp_model* m, int32_t l, const double* X, int64_t n, double* mean, double* var);

/* SVGP_Layer.conditional_ND(X, full_cov=True) (layers.py:206-209,216-219): mean (n x D_out), var (n x n x D_out). */
int dsdgp_model_layer_conditional_full(dsdgp_model* m, int32_t l, const double* X, int64_t n, double* mean, double* var);
/* utils.reparameterize, full covariance (utils.py:43-51): mean, z, out (S x n x D); var (S x n x n x D):
 * out[s,:,d] = mean[s,:,d] + chol(var[s,:,:,d] + jitter I) z[s,:,d]. */
int dsdgp_reparameterize_full(dsdgp_ctx* ctx, const double* mean, const double* var, const double* z, double jitter,
                              int64_t n, int32_t D, int32_t S, double* out);

/* utils.reparameterize, diagonal case (utils.py:40-41): out = mean + z * sqrt(var + jitter), count elements. */
int dsdgp_reparameterize(dsdgp_ctx* ctx, const double* mean, const double* var, const double* z, double jitter,
                         int64_t count, double* out);

/* N(0,1) float64 draws (Philox4x32-10 + Box–Muller), replaces tf.random_normal (layers.py:101-102). */
int dsdgp_randn(dsdgp_ctx* ctx, uint64_t seed, uint64_t stream, int64_t count, double* out);

/* Bucketed exchange of the row-sharded ELBO's gradient.  With a callback set, dsdgp_model_elbo(with_grad = 1) finishes
 * every layer's gradient right behind that layer's weight-gradient products — reduction, products, assembly, hyper-parameter sums —
 * and calls `fn(user, bucket, ptr, count, stream)` on the calling host thread as soon as the kernels that produce the bucket are
 * ENQUEUED: bucket = L-1, L-2, ..., 0 (layer l's contiguous segment of `grad`), then bucket = L (likelihood-variance entry + the four
 * result scalars when `out` = grad + n_theta; else the entry, then bucket L+1 = the scalars).  `stream` is the HIP stream the segment is
 * produced on: a collective enqueued there (ncclAllReduce(ptr, ptr, count, ncclDouble, ncclSum, comm, stream), or a torch.distributed
 * call under torch.cuda.ExternalStream(stream)) is ordered behind its producers and runs UNDER the backward chains of the layers
 * below.  The caller makes its optimiser step wait for the collectives it issued.  fn = NULL restores the single flat buffer
 * (one dsdgp_allreduce).  Ignored for white=True / wide-input models and while dsdgp_model_set_grad_first_layer restricts the pass. */
typedef void (*dsdgp_bucket_fn)(void* user, int32_t bucket, double* ptr, int64_t count, void* stream);
int dsdgp_model_set_bucket_callback(dsdgp_model* m, dsdgp_bucket_fn fn, void* user);

/* Multi-GPU exchange step of the row-sharded ELBO (the step being sharded is dgp.py:92-98): in-place SUM of
 * `count` doubles of `buf` over the ranks of `comm` on the ctx stream — ONE call per training step on the flat
 * [gradient (n_theta) | elbo, data term, kl_weight * KL, potrf_info] buffer (`grad` of dsdgp_model_create with `out` of
 * dsdgp_model_elbo pointing at grad + n_theta), between dsdgp_model_elbo(with_grad = 1, kl_weight = 1 / world,
 * data_scale = num_data / (n_local * world)) and dsdgp_model_adam_step.
 * comm: an RCCL communicator (ncclComm_t, one rank per GPU / process) created by the CALLER with RCCL's own
 * ncclGetUniqueId / ncclCommInitRank; the library resolves ncclAllReduce from the RCCL already loaded in the process (or
 * librccl.so) at first use, so libdsdgp.so itself carries no link-time dependency on RCCL.  Asynchronous.
 * Returns DSDGP_ERR_RCCL when RCCL is unavailable or reports an error (see dsdgp_last_error). */
int dsdgp_allreduce(dsdgp_ctx* ctx, void* comm, double* buf, int64_t count);

/* Minibatch gather ([UPSTREAM] gpflow.params.Minibatch, dgp.py:51-52): dst[i,:] = src[idx[idx_offset+i],:], cols wide.
 * idx: device int64.  Index generation stays on the host (own RNG; TF's shuffle order is not reproducible). */
int dsdgp_gather_rows(dsdgp_ctx* ctx, const double* src, int64_t cols, const int64_t* idx, int64_t n, int64_t idx_offset,
                      double* dst);
/* The X and Y minibatches of one step in one launch (the two Minibatch iterators of dgp.py:51-52 share their seed). */
int dsdgp_gather_rows2(dsdgp_ctx* ctx, const double* srcX, int64_t colsX, double* dstX, const double* srcY, int64_t colsY,
                       double* dstY, const int64_t* idx, int64_t n, int64_t idx_offset);

/* DGP_Base.E_log_p_Y with the Gaussian likelihood (dgp.py:83-90): out[i,d] = mean_s varexp(mean[s,i,d], var[s,i,d], Y[i,d]).
 * mean/var: (S*n x DY); Y, out: (n x DY); lik_var: host scalar.
 * sample_w (device, S doubles, may be NULL): DGP_Quad.E_log_p_Y (dgp.py:160-166) — out = sum_s sample_w[s] varexp_s
 * instead of the mean over s. */
int dsdgp_gauss_var_exp(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n, int32_t S,
                        int32_t DY, double lik_var, const double* sample_w, double* out);
/* DGP_Base.predict_density, Gaussian (dgp.py:121-126): out[i,d] = logsumexp_s log N(Y | mean, var + lik_var) - log S. */
int dsdgp_gauss_predict_density(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n,
                                int32_t S, int32_t DY, double lik_var, double* out);
/* [UPSTREAM] MultiClass(K)/RobustMax through BroadcastingLikelihood (utils.py:76-93):
 * mode 0: out[i] = mean_s variational expectation ; mode 1: out[i] = logsumexp_s log density - log S.
 * mean/var: (S*n x K); Y: (n x 1) class labels stored as doubles; out: (n x 1). */
int dsdgp_multiclass_var_exp(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n, int32_t S,
                             int32_t K, int mode, const double* sample_w, double* out);
/* MultiClass.predict_mean_and_var: out_mean[r,k] = predictive class probability, out_var = p - p^2; R rows. */
int dsdgp_multiclass_predict(dsdgp_ctx* ctx, const double* mean, const double* var, int64_t R, int32_t K, double* out_mean,
                             double* out_var);

/* [UPSTREAM] Bernoulli() (probit link, 20-point Gauss-Hermite variational expectations) through BroadcastingLikelihood
 * (utils.py:76-86; exercised by /root/reference/tests/test_dgp.py:48-54).  Targets: 1 selects p, anything else 1 - p.
 * mode 0: out[i,d] = mean_s (or sum_s sample_w[s]) variational expectation ; mode 1: out[i,d] = logsumexp_s log density - log S.
 * mean/var: (S x n x DY); Y, out: (n x DY). */
int dsdgp_bernoulli_var_exp(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n, int32_t S,
                            int32_t DY, int mode, const double* sample_w, double* out);
/* Bernoulli.predict_mean_and_var (probit closed form): out_mean = probit(mean / sqrt(1 + var)), out_var = p - p^2. */
int dsdgp_bernoulli_predict(dsdgp_ctx* ctx, const double* mean, const double* var, int64_t count, double* out_mean,
                            double* out_var);

/* BroadcastingLikelihood over Poisson(invlink=exp, binsize) / Exponential(invlink=exp) / Gamma(invlink=exp; shape) /
 * StudentT(scale, deg_free) / Beta(invlink=probit, scale)
 * (utils.py:76-93,95-121; [UPSTREAM] gpflow 1.1.1 likelihoods: closed-form variational expectations with the exp link, the base
 * class's 20-point Gauss-Hermite rule otherwise).  kind = DSDGP_LIK_POISSON .. DSDGP_LIK_BETA; p0 = StudentT.scale / Gamma.shape /
 * Beta.scale, p1 = Poisson.binsize / StudentT.deg_free (ignored where the likelihood has no such parameter).  Modes, shapes: as above. */
int dsdgp_lik_var_exp(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var, const double* Y,
                      int64_t n, int32_t S, int32_t DY, int mode, const double* sample_w, double* out);
/* Likelihood.predict_mean_and_var by the same rule: E_y = sum w cm(f_k), V_y = sum w (cv(f_k) + cm(f_k)^2) - E_y^2. */
int dsdgp_lik_predict(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var, int64_t count,
                      double* out_mean, double* out_var);

/* Read-out of the likelihood launch of a training step (verification aid: nothing on the evaluation path calls it).  Launches the
 * kernel dsdgp_model_elbo ends its forward pass with — the same instance, the same grid — on caller-supplied DEVICE arrays: mean, var
 * (S x n x DY), Y (n x DY).  kind = any element-wise DSDGP_LIK_* (Gaussian and Bernoulli included); p0, p1 as for dsdgp_eval_mixture;
 * w = data_scale / S; sample_w (S doubles or NULL) = the quadrature weights of DGP_Quad.  With ve = the variational expectation of one
 * element and f = sample_w[s] S (1 without weights) it writes
 *   dmean, dvar (S n DY each, row-major; both or neither):  -w f d ve / d mean, -w f d ve / d var — the form a one-layer model reads;
 *   MBt, VBt (DY x ldt each, ldt >= S n; both or neither, and not together with dmean): the same numbers transposed, MBt[d][row], rows
 *     S n .. ldt - 1 written as +0.0 — the form the last layer's backward chain of a deeper model reads (ldt = S n rounded up to 16);
 *   part (2 x blocks doubles; blocks = ceil(S n DY / 256), with MBt ceil(ldt DY / 256)): part[2 b] = sum of f ve over the 256 elements
 *     of block b, part[2 b + 1] = sum of f d ve / d p0 (0 for the kinds without a parameter).  ELBO data term = w sum_b part[2 b].
 * Asynchronous on the ctx stream. */
int dsdgp_lik_elbo_readout(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var, const double* Y,
                           int64_t n, int32_t S, int32_t DY, double w, const double* sample_w, double* part, double* dmean,
                           double* dvar, double* MBt, double* VBt, int64_t ldt);
/* The same for MultiClass(K): ve[row] (S n) = f var_exp of row s n + i with label Y[i] (n x 1 doubles, integers in [0, K): the kernel
 * indexes with them and does not check), dmean / dvar (S n x K) = -w f d var_exp / d mean, / d var; 2 <= K <= 32.  The factor f is
 * applied by the launch that follows the likelihood kernel in a DGP_Quad step, after rounding. */
int dsdgp_multiclass_readout(dsdgp_ctx* ctx, const double* mean, const double* var, const double* Y, int64_t n, int32_t S, int32_t K,
                             double w, const double* sample_w, double* ve, double* dmean, double* dvar);

/* Held-out evaluation, the reduction of demos/run_regression.py:108-123 over the S components of DGP_Base.predict_y / predict_density
 * (dgp.py:116-126), on caller-supplied mean / var ((S*n) x DY, row s*n + i, as dsdgp_model_propagate writes them) and Y (n x DY;
 * MultiClass: n x 1 labels, DY = K).  With (E_s, V_s) = predict_mean_and_var of component s, per (i, d):
 *   mhat = mean_s E_s ;  mixture variance = mean_s (V_s + E_s^2) - mhat^2 ;  l = logsumexp_s log p(y | mean_s, var_s) - log S
 * (S = 1: the component's own values, exactly).  kind = any DSDGP_LIK_*; p0 = Gaussian.variance / StudentT.scale / Gamma.shape /
 * Beta.scale, p1 = Poisson.binsize / StudentT.deg_free (ignored where the likelihood has no such parameter).
 *   rows_out (device, n x DY x 3, or NULL): [mhat, mixture variance, l] per (i, d); MultiClass: per class k its mixture probability
 *            and that probability's variance, l of the row repeated for every k.
 *   acc (device, 3*DY doubles): acc[d] = sum_i (Y - mhat)^2, acc[DY + d] = sum_i l, acc[2*DY + d] = n — overwritten, or added to when
 *            accumulate != 0 (batches; the sums of data-parallel ranks add up).  MultiClass: d = 0 only (the other entries stay 0), with
 *            acc[0] = the number of rows whose argmax_k mhat_k (ties: the lowest k) differs from the label.
 * Fixed-order reductions: the same inputs and n give the same bits.  DSDGP_ERR_UNSUPPORTED for a kind outside DSDGP_LIK_* or K > 32. */
int dsdgp_eval_mixture(dsdgp_ctx* ctx, int32_t kind, double p0, double p1, const double* mean, const double* var, const double* Y,
                       int64_t n, int32_t S, int32_t DY, double* rows_out, double* acc, int accumulate);
/* The same on a model's own predictions: the forward pass of dsdgp_model_propagate (same kernels, same Philox draws from `seed`, same
 * `zs` injection) with only the last layer's mean and variance kept, in the workspace, then dsdgp_eval_mixture on them with the
 * model's likelihood — one batch of the loop of demos/run_regression.py:108-123 without a copy to the host.  X (n x D_in0), Y as above.
 * DSDGP_ERR_UNSUPPORTED while quadrature sample weights are set (dsdgp_model_set_sample_weights). */
int dsdgp_model_evaluate(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                         const int64_t* zstride, uint64_t seed, double* rows_out, double* acc, int accumulate);

/* Calibration of the predictive mixture of dgp.py:116-126: S Gaussians N(mean_s, var_s + noise_var) per (i, d), equally weighted, on
 * caller-supplied mean / var ((S*n) x DY, row s*n + i, as dsdgp_model_propagate writes them).  With sig_s^2 = max(var_s + noise_var,
 * DBL_MIN) and F(x) = (1/S) sum_s Phi((x - mean_s) / sig_s):
 *
 * dsdgp_mixture_quantiles: q_out (device, n x DY x P) = the roots of F(q) = probs[k] — the exact credible-interval ends that
 * demos/using_natural_gradients.ipynb cell 9 estimates by np.percentile(samples, [10, 50, 90]) of 100 full-covariance draws, and that
 * demos/demo_step_function.ipynb:83-85 and demos/priors.ipynb:1020 replace by mean +- 1.96 sqrt(var) of a single Gaussian.
 * probs: HOST array of P probabilities, 0 < p < 1, 1 <= P <= 16, copied into the launch (no upload, no synchronisation).  Safeguarded
 * Newton inside a bracket that holds the root, at most 128 steps per probability (at the cap: the bracket's midpoint). */
int dsdgp_mixture_quantiles(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, int64_t n, int32_t S, int32_t DY,
                            const double* probs, int32_t P, double* q_out);
/* dsdgp_mixture_calibration: the scores of held-out targets Y (device, n x DY) under the same mixture (dgp.py:116-126; the host route is
 * predict_y, two (S, N*, D) downloads and numpy).  Per (i, d): the probability integral transform u = F(y) and the continuous ranked
 * probability score in closed form (Grimit et al. 2006), with A(m, s^2) = m (2 Phi(m/s) - 1) + 2 s phi(m/s):
 *   CRPS = (1/S) sum_s A(y - mean_s, sig_s^2) - (1/(2 S^2)) sum_s sum_t A(mean_s - mean_t, sig_s^2 + sig_t^2).
 *   rows_out (device, n x DY x 2, or NULL): [u, CRPS] per (i, d).
 *   acc (device, (2 + P)*DY doubles): acc[d] = sum_i CRPS, acc[DY + d] = n, acc[(2 + k)*DY + d] = the number of rows with u <= probs[k]
 *            (exact integers) — overwritten, or added to when accumulate != 0 (batches; data-parallel ranks).
 * Fixed-order reductions: the same inputs and n give the same bits.  DSDGP_ERR_BAD_ARG for a probability outside (0, 1), P outside
 * 1..16 or a negative noise_var. */
int dsdgp_mixture_calibration(dsdgp_ctx* ctx, const double* mean, const double* var, double noise_var, const double* Y, int64_t n,
                              int32_t S, int32_t DY, const double* probs, int32_t P, double* rows_out, double* acc, int accumulate);
/* The same on a model's own predictions: the forward pass exactly as dsdgp_model_evaluate runs it (same kernels, same Philox draws from
 * `seed`, same `zs` injection, only the last layer's mean and variance kept, in the workspace), then the primitive on the same stream —
 * one batch of what demos/using_natural_gradients.ipynb cell 9, demos/demo_step_function.ipynb:83-85 and demos/priors.ipynb:1020 do on
 * the host.  level 0: the latent f (noise 0), every likelihood; level 1: the predictive y, noise = the Gaussian likelihood's variance
 * read from the model's device copy.  DSDGP_ERR_UNSUPPORTED for level 1 / dsdgp_model_calibration with any other likelihood, and while
 * quadrature sample weights are set (dsdgp_model_set_sample_weights). */
int dsdgp_model_quantiles(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs, const int64_t* zstride,
                          uint64_t seed, int32_t level, const double* probs, int32_t P, double* q_out);
int dsdgp_model_calibration(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                            const int64_t* zstride, uint64_t seed, const double* probs, int32_t P, double* rows_out, double* acc,
                            int accumulate);

/* Classification report of the predictive mixture of dgp.py:116-126 for the two likelihoods with classes, on caller-supplied mean / var
 * ((S*n) x DY, row s*n + i, as dsdgp_model_propagate writes them): is the classifier calibrated, and which classes does it confuse?
 *   kind = DSDGP_LIK_MULTICLASS: Y (device, n x 1) labels, DY = K classes, 2 <= K <= 32, C = K, ND = 1.  pi[i, k] = (1/S) sum_s p_{s,i,k},
 *          p_{s,i,k} the RobustMax predictive probability of class k by the arithmetic of dsdgp_multiclass_predict, all K classes of all S
 *          components in ONE launch (no (S n)-sized intermediate goes through memory).
 *   kind = DSDGP_LIK_BERNOULLI: Y (device, n x DY), every output d its own two-class problem (class 1: Y == 1, class 0: any other target),
 *          C = 2, ND = DY.  p[i, d] = (1/S) sum_s probit(mean_s / sqrt(1 + var_s)), pi = (1 - p, p).
 * Per row i (Bernoulli: per (i, d)), with the label y clamped into 0 .. C-1: predicted class c^ = argmax_c pi_c (ties: the lowest c, so a
 * Bernoulli p of exactly 0.5 predicts class 0), conf = pi_c^, l = log pi_y (the log density of dsdgp_eval_mixture),
 * brier = sum_c (pi_c - [c = y])^2 (the multi-class definition: a binary problem gives 2 (p - t)^2, twice the usual binary Brier score),
 * rank = #{c : pi_c > pi_y} + #{c < y : pi_c == pi_y}, bin = min(bins - 1, floor(conf * bins)): `bins` equal-width bins on [0, 1].
 *   bins: 1 .. 32.
 *   probs_out (device, n x DY, or NULL): pi (MultiClass), p(y = 1) (Bernoulli).
 *   rows_out (device, n x ND x 4, or NULL): [c^, conf, l, brier].
 *   acc (device, E*ND doubles, E = 4 + 3*bins + C + C*C), entry acc[q*ND + d]:
 *            q = 0 sum [c^ != y], 1 sum l, 2 sum brier, 3 rows; 4 + b rows in bin b; 4 + bins + b sum of conf over bin b;
 *            4 + 2*bins + b sum of [c^ = y] over bin b; 4 + 3*bins + r rows whose label has rank r;
 *            4 + 3*bins + C + t*C + c rows with label t predicted as c
 *            — the counts exact integers; overwritten, or added to when accumulate != 0 (batches; data-parallel ranks).
 * Fixed-order reductions: the same inputs and n give the same bits.  DSDGP_ERR_UNSUPPORTED for any other kind or K outside 2..32,
 * DSDGP_ERR_BAD_ARG for bins outside 1..32. */
int dsdgp_mixture_classification(dsdgp_ctx* ctx, int32_t kind, const double* mean, const double* var, const double* Y, int64_t n,
                                 int32_t S, int32_t DY, int32_t bins, double* probs_out, double* rows_out, double* acc, int accumulate);
/* The same on a model's own predictions: the forward pass exactly as dsdgp_model_evaluate runs it (same kernels, same Philox draws from
 * `seed`, same `zs` injection, only the last layer's mean and variance kept, in the workspace), then the primitive on the same stream with
 * the model's likelihood.  DSDGP_ERR_UNSUPPORTED for a model whose likelihood is neither MultiClass nor Bernoulli, and while quadrature
 * sample weights are set (dsdgp_model_set_sample_weights). */
int dsdgp_model_classification(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                               const int64_t* zstride, uint64_t seed, int32_t bins, double* probs_out, double* rows_out, double* acc,
                               int accumulate);

/* dsdgp_kmeans: Lloyd's k-means for the inducing points, Z = kmeans2(X, M, minit='points')[0] of demos/run_regression.py:57 (scipy, one
 * host thread) on the device.  X (device, n x D, row-major), Z0 (device, M x D): the initial centres (with minit='points', M rows of X).
 * `iters` iterations of  assign: label_i = argmin_m |x_i - z_m|^2 (ties: the lowest m; a NaN never wins, so 0 <= label < M whatever X
 * holds),  update: z_m = the mean of the rows labelled m; a centre without rows keeps its value bit for bit (kmeans2's missing='warn',
 * without the warning).  All of them are enqueued on the context's stream; the host does not wait.
 *   Z (device, M x D): the centres after the last update; may alias Z0.
 *   labels (device, n x int32, or NULL), counts (device, M x int64, or NULL), inertia (device, 1 double, or NULL): the last assignment —
 *            the one Z was averaged from, what kmeans2 returns as its labels — its cluster sizes and its sum_i min_m |x_i - z_m|^2.
 * The arithmetic runs on X minus its column means (k-means is translation-invariant; |x|^2 + |z|^2 - 2 x.z on uncentred data is not),
 * the cross products on the fp64 MFMA pipe with the argmin fused behind them: nothing of size n x M reaches memory.  Every reduction runs
 * in a fixed order and the update sorts the rows by label instead of adding with floating-point atomics: the same X, Z0 and iters give
 * the same bits, on every rank of a data-parallel run.
 * DSDGP_ERR_BAD_ARG (nothing launched, Z untouched) for n < M, n >= 2^31, M outside 2..2048, D outside 1..1024, iters < 1 or a NULL
 * X / Z0 / Z. */
int dsdgp_kmeans(dsdgp_ctx* ctx, const double* X, int64_t n, int32_t D, int32_t M, const double* Z0, int32_t iters, double* Z,
                 int32_t* labels, int64_t* counts, double* inertia);

/* dsdgp_greedy_inducing: greedy conditional-variance selection of the inducing points — the pivoted Cholesky factorisation of
 * K(X, X) ("ConditionalVariance" of Burt, Rasmussen and van der Wilk 2020) on the device.  X (device, n x D, row-major, D =
 * kern->input_dim); kern as for dsdgp_gram (RBF or Matern52, scalar or ARD lengthscales, optional White part).
 *   d_i = kern.Kdiag (variance + white_variance);  for j = 0 .. M-1:  p_j = `first` if j == 0 and first >= 0, else argmax_i d_i over the
 *   rows not yet chosen (ties: the lowest i; a NaN never wins);  stop if d_p <= threshold (m = j points);  c_j[i] = (k(x_i, x_p) -
 *   sum_{t<j} c_t[i] c_t[p]) / sqrt(d_p);  d_i = max(d_i - c_j[i]^2, 0), d_p = 0;  trace_j = sum_i d_i = tr(Kff - Qff) of the first j + 1 points.
 * All M steps are enqueued on the context's stream; the host does not wait and the chosen row never visits it.
 *   idx (device, M x int32): p_0 .. p_{m-1};  m_out (device, 1 x int32): m.
 *   Z (device, M x D, or NULL): the chosen rows, bit copies of rows of X;  residual (device, M, or NULL): d_p at the time row p was
 *   chosen;  trace (device, M, or NULL): trace_j;  L (device, M x ldl, or NULL): L[j][t] = c_t[p_j] (t < j), L[j][j] = sqrt(residual_j),
 *   zero above — the lower Cholesky factor of k(Z, Z) (+ white_variance I) in pivot order; the columns M .. ldl of L are not written.
 *   Entries j >= m after an early stop: idx -1, residual 0, trace = trace_{m-1} (tr K(X, X) if m = 0), zero rows of Z and L.
 * r^2 is formed from differences of rows, never from |x|^2 + |z|^2 - 2 x.z.  Every sum runs in a fixed order (sum_t ascending in t, no
 * floating-point atomics) and a row's arithmetic does not depend on where the row sits: the same arguments give the same bits on every
 * call and every rank, and two bit-identical rows of X tie exactly (the lower index wins).  Step j moves 8 n (D + j + 3) bytes.
 * DSDGP_ERR_BAD_ARG (nothing launched, no output touched) for n < M, n >= 2^31, M outside 2..2048, kern->input_dim outside 1..1024, a
 * kind other than RBF / Matern52, first outside -1 .. n-1, a negative or NaN threshold, a NULL X / idx / m_out, or L with ldl < M.
 * DSDGP_ERR_UNSUPPORTED when the M x n column store (or the D x n transposed copy of X) would exceed 2^30 doubles (8 GB of scratch):
 * pass a subset of the rows. */
int dsdgp_greedy_inducing(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int32_t M, int64_t first,
                          double threshold, int32_t* idx, int32_t* m_out, double* Z, double* residual, double* trace, double* L,
                          int64_t ldl);

/* dsdgp_pca: the PCA behind the step-down mean functions — the top k right singular vectors of X, which the reference's
 * init_layers_linear takes from np.linalg.svd(X, full_matrices=False) (layer_initializations.py:35) — as the top k eigenvectors of
 * the D x D matrix C on the device.  X (device, n x D, row-major).
 *   center = 0: C = X^T X (what svd(X) diagonalises; the reference does not centre);  center = 1: C = (X - 1 mean^T)^T (X - 1 mean^T),
 *   mean = the column means, subtracted from the rows as they are staged (X^T X - n mean mean^T is never formed).
 *   C = V diag(lambda) V^T by two-sided Jacobi in the round-robin ordering (D padded to even, D - 1 or D steps of disjoint pairs per sweep):
 *   pair (p, q) is skipped when |a_pq| <= 2^-53 sqrt(|a_pp a_qq|), else theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| +
 *   sqrt(theta^2 + 1)), sgn(0) = 1.  After each sweep off = sqrt(sum_{i != j} a_ij^2) is measured from the entries themselves; the
 *   iteration has converged when off <= D 2^-52 |C|_F or a sweep rotated nothing.  max_sweeps sweeps are enqueued; the steps after
 *   convergence return at once.
 *   W (device, D x ldw): column j < k = the unit eigenvector of the j-th largest eigenvalue, its entry of largest magnitude positive (ties:
 *            the lowest row); the columns k .. ldw are not written.
 *   evals (device, D, or NULL): all D eigenvalues, non-increasing; equal eigenvalues keep the order of their index in the solver's diagonal.
 *   mean (device, D, or NULL): the column means (center = 1) or zeros (center = 0).
 *   gram (device, D x D, or NULL): C as the device formed it, exactly symmetric.
 *   info (device, 4 x int32, or NULL): {converged, sweeps run, rotations applied in the last sweep, 0}.
 * Everything is enqueued on the context's stream; the host does not wait.  C is formed on the fp64 MFMA pipe from the 64 x 64 tiles on or
 * below its diagonal, the rows of X split over workgroups and the partial tiles added in ascending split order; no floating-point atomics
 * anywhere and no kernel waits for another workgroup: the same X, k, center and max_sweeps give the same bits on every call and every
 * rank.  The Gram launch reads 8 n 128 bytes of X per off-diagonal tile (8 n 64 per diagonal one, mostly from L2) and writes 32 KB per
 * (tile, split); a Jacobi step reads and writes the two Dp x Dp matrices A and V once: 32 Dp^2 bytes.
 * DSDGP_ERR_BAD_ARG (nothing launched, no output touched) for n < 1, n >= 2^31, D outside 1..1024, k outside 1..D, center outside {0, 1},
 * max_sweeps outside 1..64, ldw < k or a NULL X / W.  DSDGP_ERR_UNSUPPORTED if the partial tiles of one row split exceeded 256 MB of
 * scratch (they are 4.5 MB at D = 1024; the number of splits is chosen so that all of them stay below that cap). */
int dsdgp_pca(dsdgp_ctx* ctx, const double* X, int64_t n, int32_t D, int32_t k, int32_t center, int32_t max_sweeps, double* W, int64_t ldw,
              double* evals, double* mean, double* gram, int32_t* info);

/* dsdgp_rbf_expectations: the expectations of an RBF kernel under a diagonal Gaussian input (the psi statistics) that the reference's
 * collapsed layers take from GPflow 1.1.1's expectation(DiagonalGaussian, (RBF, InducingPoints)[, (RBF, InducingPoints)])
 * (layers.py:415-417, 494-495).  mu, s (device, n x D): means and variances of the rows, s == NULL: zero variance; Z (device, M x D);
 * kern as for dsdgp_gram, D = kern->input_dim, variance v, lengthscales l_d (scalar or ARD).
 *   psi0 (device, 1 double, or NULL)      = n v
 *   psi1 (device, n x ld1, or NULL)[r, i] = v prod_d (l_d^2 / (l_d^2 + s_rd))^1/2 exp(-1/2 sum_d (mu_rd - z_id)^2 / (l_d^2 + s_rd))
 *   psi2 (device, M x ld2, or NULL)[i, j] = sum_r v^2 prod_d (l_d^2 / (l_d^2 + 2 s_rd))^1/2
 *                                           exp(-sum_d [(z_id - z_jd)^2 / (4 l_d^2) + (mu_rd - (z_id + z_jd) / 2)^2 / (l_d^2 + 2 s_rd)])
 * The columns M .. ld of psi1 and psi2 are not written.  Every exponent is formed from differences of the inputs, never from an
 * expanded square; for s >= 0 every term of an exponent is <= 0, so a far pair underflows to +0.  s is not clamped: a row with
 * l_d^2 + 2 s_rd < 0 gives NaN in the entries it feeds, as upstream's sqrt does.  psi2 is n M (M + 1) / 2 exponentials: only the 16 x 16
 * tiles on or below the diagonal are formed (the mirror image is written with them: psi2 is exactly symmetric), the rows split over
 * workgroups, the term sum_d t_rd (z_id - z_jd)^2 of the exponent on the fp64 MFMA pipe, and the partial tiles added in ascending split
 * order — no floating-point atomics: the same arguments give the same bits on every call.  Asynchronous on the context's stream; the
 * row tables (8 n (3 D + M + 6) bytes) live in the context's scratch.
 * DSDGP_ERR_UNSUPPORTED for a kernel that is not RBF or has a White part (Matern52 has no closed form), or when the row tables would
 * exceed 8 GB (pass the rows in batches and add the results).  DSDGP_ERR_BAD_ARG for M outside 1..2048, n < 1, n >= 2^31,
 * kern->input_dim outside 1..1024, ld1 / ld2 < M or a NULL kern / Z / mu. */
int dsdgp_rbf_expectations(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu, const double* s,
                           int64_t n, double* psi0, double* psi1, int64_t ld1, double* psi2, int64_t ld2);

/* dsdgp_rbf_expectations_grad: the reverse pass of dsdgp_rbf_expectations — what tf.gradients builds through
 * expectation(DiagonalGaussian, (RBF, InducingPoints)[, (RBF, InducingPoints)]) (layers.py:415-417) when the reference's demos and tests
 * fit a collapsed model with ScipyOptimizer().minimize(m) (tests/test_collapsed.py:10, tests/test_dgp.py:150).  Given the adjoints g_psi0 (a number),
 * g_psi1 (device, n x ldg1, or NULL: zero) and g_psi2 (device, M x ldg2, or NULL: zero; need not be symmetric: (g + g^T) / 2 is what
 * acts) of a scalar F, it OVERWRITES
 *   d_mu, d_s (device, n x D)   dF/dmu, dF/ds   (s == NULL: the derivative at s = 0)
 *   d_Z (device, M x D)         dF/dZ
 *   d_kern (device)             [0] = dF/d variance, [1 ..] = dF/d lengthscales: D entries with ARD, else one
 * every one of them optional (NULL).  kern: a plain RBF kernel with input_dim <= 32 (one chunk of the forward's operand).  The psi2
 * part recomputes the forward's exponent from the forward's own row tables rather than store n M^2 values: a workgroup owns a tile row
 * of 16 inducing inputs and a split of the rows and walks every tile column (n M^2 exponentials), the exponent's sum_d t_rd Delta_ijd^2
 * and the two contractions of the weighted terms over the pairs on the fp64 MFMA pipe; every difference is formed as a difference of
 * the inputs.  No floating-point atomics, every summation order depends on (n, M, D) alone: the same arguments give the same bits.  A
 * row with l_d^2 + 2 s_rd < 0 gives NaN in its own rows of d_mu and d_s and in every output that sums over rows; a pair whose
 * exponential underflows contributes +0.  Asynchronous on the context's stream; the tables (8 n (3 M + (M / 16 + 5) D + 8) bytes at
 * most) live in the context's scratch.
 * DSDGP_ERR_UNSUPPORTED for a kernel that is not RBF or has a White part, for input_dim > 32, or when the tables would exceed 8 GB (pass
 * the rows in batches and add the results).  DSDGP_ERR_BAD_ARG for M outside 1..2048, n < 1, n >= 2^31, kern->input_dim outside
 * 1..1024, ldg1 / ldg2 < M or a NULL kern / Z / mu.  A refused call launches nothing. */
int dsdgp_rbf_expectations_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu, const double* s,
                                int64_t n, double g_psi0, const double* g_psi1, int64_t ldg1, const double* g_psi2, int64_t ldg2,
                                double* d_mu, double* d_s, double* d_Z, double* d_kern);

/* The small steps of the reference's collapsed bound and its prediction (gplvm_build_likelihood / gplvm_build_predict, psi branch,
 * layers.py:405-450, 483-525) that the primitives above lack; SGPR_Layer of the host mirror composes them with dsdgp_gram, dsdgp_potrf,
 * dsdgp_trsm and dsdgp_gemm.  All asynchronous; every sum in a fixed order.
 * dsdgp_scale_copy: B (m x n) = op(A) / div + diag_add I, op(A) = A (trans = 0) or A^T (trans = 1) — tf.transpose(tmp) of layers.py:426,
 * AAT / sigma2 and AAT + eye of :426-427.  A and B must not overlap. */
int dsdgp_scale_copy(dsdgp_ctx* ctx, int trans, int m, int n, const double* A, int64_t lda, double div, double diag_add, double* B,
                     int64_t ldb);
/* dsdgp_collapsed_bound: the terms of layers.py:443-448 from LB = chol(AAT + I) (M x ldb), G = L^-1 psi2 L^-T (M x ldg; AAT = G /
 * noise_var), c (M x DY), Y (n x DY), psi0 (device scalar) and the likelihood's noise variance.  out (device, 7 doubles): out[0] = the
 * bound, out[1..6] = -1/2 n DY log(2 pi noise_var), -DY sum log diag(LB), -1/2 sum Y^2 / noise_var, 1/2 sum c^2,
 * -1/2 DY psi0 / noise_var, 1/2 DY tr(G) / noise_var;  out[0] adds them in this order. */
int dsdgp_collapsed_bound(dsdgp_ctx* ctx, int32_t M, int64_t n, int32_t DY, const double* LB, int64_t ldb, const double* G, int64_t ldg,
                          const double* c, const double* Y, const double* psi0, double noise_var, double* out);
/* dsdgp_collapsed_var: var[r, d] = kdiag + sum_m tmp2[m, r]^2 - sum_m tmp1[m, r]^2 for every output d < DY (layers.py:521-524);
 * tmp1 = L^-1 K(Z, X*), tmp2 = LB^-1 tmp1 (M x ld, ns columns used), var (ns x DY). */
int dsdgp_collapsed_var(dsdgp_ctx* ctx, int32_t M, int64_t ns, int32_t DY, const double* tmp1, int64_t ld1, const double* tmp2,
                        int64_t ld2, double kdiag, double* var);
/* dsdgp_collapsed_adjoints: the adjoints of the bound of layers.py:443-448, read as F(Kuu, psi0, psi1, psi2, noise_var), that
 * tf.gradients forms when a collapsed model is fitted (tests/test_collapsed.py:10, tests/test_dgp.py:150), from the dense M x M matrices (leading dimension
 * M) Si = Sigma^-1 with Sigma = Kuu + psi2 / noise_var, Ki = Kuu^-1, KpK = Ki psi2 Ki, psi2, and alpha = Sigma^-1 psi1^T Y / noise_var,
 * c (both M x DY), Y (n x DY), psi0 (device scalar).  With dS = -1/2 DY Si - 1/2 alpha alpha^T:
 *   g_psi2 (M x M) = dS / noise_var + 1/2 DY Ki / noise_var,   d_Kuu (M x M) = dS + 1/2 DY Ki - 1/2 DY KpK / noise_var,
 *   out (device, 8 doubles): out[0] = dF/d noise_var, out[1..6] its terms -1/2 n DY / s2, 1/2 sum Y^2 / s2^2, -sum c^2 / s2,
 *   1/2 DY psi0 / s2^2, -1/2 DY tr(Ki psi2) / s2^2, -tr(dS psi2) / s2^2 (added in this order), out[7] = g_psi0 = -1/2 DY / s2.
 * (g_psi1 = Y alpha^T / noise_var is one dsdgp_gemm.)  One workgroup, every sum in a fixed order; asynchronous. */
int dsdgp_collapsed_adjoints(dsdgp_ctx* ctx, int32_t M, int64_t n, int32_t DY, const double* Si, const double* Ki, const double* KpK,
                             const double* psi2, const double* alpha, const double* c, const double* Y, const double* psi0,
                             double noise_var, double* g_psi2, double* d_Kuu, double* out);

/* dsdgp_gram_grad: the reverse pass of dsdgp_gram — what tf.gradients builds through kern.K when the reference fits or samples a model of
 * dense layers (GPMC_Layer, GPR_Layer: layers.py:263-293, 310-342; DGP_Heinonen, model_zoo.py:60-88), whose bound depends on its inputs
 * only through K(F, F).  Same kernels as dsdgp_gram: RBF or Matern52, scalar or ARD lengthscales, optional White part.  G (device,
 * n x ldg) is the adjoint of dsdgp_gram's output for a scalar F; every output is optional (NULL) and is OVERWRITTEN:
 *   cross form (X2 != NULL):       d_X[i, :]  = sum_j G_ij dk(x_i, y_j)/dx_i   (n x D),    d_X2[j, :] = sum_i G_ij dk(x_i, y_j)/dy_j   (n2 x D)
 *   symmetric form (X2 == NULL, K = k(X, X) + (white_variance + jitter) I; G need not be symmetric; d_X2 must be NULL):
 *                                  d_X[i, :]  = sum_j (G_ij + G_ji) dk(x_i, x_j)/dx_i
 *   d_kern (device, 2 + (ard ? D : 1) doubles): [0] = dF/d variance, [1 ..] = dF/d lengthscales (D entries with ARD, else one), then one
 *                                  more entry, dF/d(diagonal add) = sum_i G_ii: written in the symmetric form, 0 in the cross form.  It is at
 *                                  once the gradient in the White variance and in whatever the caller passed to dsdgp_gram as `jitter`
 *                                  (GPR_Layer passes the noise variance there).
 * With r2 = sum_d ((x_d - y_d) / l_d)^2 and dk/dr2 of the forward's kernel function (Matern52 with its r = sqrt(r2 + 1e-12)):
 * dk/dx_d = 2 (x_d - y_d) / l_d^2 dk/dr2, dk/dl_d = -2 (x_d - y_d)^2 / l_d^3 dk/dr2.  Every x_d - y_d is formed as a difference of the
 * inputs, never from an expanded square.  Coincident rows give a finite, zero contribution; a pair whose exponential underflows
 * contributes +0.  One thread holds one row, the other side is walked in tiles staged in the LDS; rows are split over workgroups, column
 * ranges over splits, partial results are added in ascending split order.  No floating-point atomics; every summation order depends on
 * (n, n2, D, form) alone: the same arguments give the same bits, and an output requested alone has the bits it has when all are
 * requested.  Asynchronous on the context's stream; the partial sums live in the context's scratch.
 * DSDGP_ERR_UNSUPPORTED for input_dim > 32 (as for dsdgp_rbf_expectations_grad) or more than 8 GB of partial sums.  DSDGP_ERR_BAD_ARG for
 * n or n2 outside 1 .. 2^31 - 1, ldg < n2 (n in the symmetric form), a kernel kind other than the two, input_dim < 1, a NULL ctx / kern /
 * X / G, or d_X2 != NULL in the symmetric form.  A refused call launches nothing. */
int dsdgp_gram_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, const double* X2, int64_t n2, const double* G,
                    int64_t ldg, double* d_X, double* d_X2, double* d_kern);

/* The two small steps of the reference's dense collapsed layer (GPR_Layer, layers.py:310-342) that the primitives above lack; GPR_Layer
 * of the host mirror composes them with dsdgp_gram (the noise variance as its diagonal add), dsdgp_potrf, dsdgp_trsm and dsdgp_gemm.
 * Both asynchronous; every sum in a fixed order.
 * dsdgp_gpr_bound: multivariate_normal(Y, m, L) of layers.py:342 summed over the outputs, from L = chol(K + noise_var I) (device,
 * n x ldl, the diagonal is read) and V = L^-1 (Y - m) (device, n x ldv, DY columns used).  out (device, 4 doubles): out[0] = the bound,
 * out[1..3] = -1/2 n DY log(2 pi), -DY sum log L_ii, -1/2 sum V^2;  out[0] adds them in this order.  One workgroup. */
int dsdgp_gpr_bound(dsdgp_ctx* ctx, int64_t n, int32_t DY, const double* L, int64_t ldl, const double* V, int64_t ldv, double* out);
/* dsdgp_gpr_var: var[r, d] = kdiag - sum_i A[i, r]^2 for every output d < DY (layers.py:333-334); A = L^-1 K(F, X*) (n x lda, ns columns
 * used), var (ns x DY).  An entry point of its own rather than dsdgp_collapsed_var, which would need an n x ns matrix of zeros as its
 * second operand. */
int dsdgp_gpr_var(dsdgp_ctx* ctx, int64_t n, int64_t ns, int32_t DY, const double* A, int64_t lda, double kdiag, double* var);

/* dsdgp_sparse_conditional / dsdgp_sparse_conditional_grad: the reference's sparse conditional on the branch `q_sqrt is None`
 * (layers.py:178-219, line 200), which is all of its SGPMC_Layer (layers.py:249-260), and the reverse pass tf.gradients builds through it.
 * kern: RBF or Matern52, scalar or ARD lengthscales, with or without a White part; Z (M x D), X (n x D), q_mu (M x DO): device.  With
 *   Ku = K(Z, Z) + jitter I (White on the diagonal, as dsdgp_gram's symmetric form),  Lu = chol(Ku),  A = Lu^-1 K(Z, X),
 *   W = q_mu (white != 0) or Lu^-1 q_mu,  kd = variance + White variance:
 *   mean (n x DO) = A^T W,   var (n) = kd - sum_i A_ir^2 in ascending i: ONE column, the reference gives every output the same variance.
 * Reverse, given gm = dJ/dmean (n x DO) and gv = dJ/dvar already summed over the outputs (n), every output optional and OVERWRITTEN:
 *   d_q_mu (M x DO);  d_Z (M x D);  d_X (n x D);  d_kern (2 + (ard ? D : 1) doubles): variance, lengthscales, then the gradient in what is
 *   added to Ku's diagonal — with a White part the White variance, which also takes kd's adjoint sum_r gv_r; without one the jitter.
 * The Gram matrices, the factorisation, the solves, the M x M products and the two Gram reverse passes are this library's own calls; the
 * passes over the M x n matrix A are two kernels of their own (csrc/sparse_cond.hip): one read of a tile of A gives mean and var, one read
 * gives A_bar and the tile's part of A gm.  No floating-point atomics; every summation order follows from (n, M, D, DO) alone
 * (csrc/sparse_cond_plan.hpp): the same call gives the same bits, whichever outputs are asked for.
 * SCRATCH: the composed calls use the context's scratch, so the intermediates live in a block the CALLER holds: `scratch` (device, 256-byte
 * aligned) of at least dsdgp_sparse_conditional_scratch_bytes(n, M, D, DO, reverse) bytes.  No state is saved between the two calls: the
 * reverse call repeats the forward's factorisation and solves itself.
 * info (host, may be NULL): the Cholesky status, as dsdgp_potrf; a failed factorisation returns DSDGP_ERR_NOT_SPD and writes no output.
 * M <= 2048.  The forward takes any input_dim dsdgp_gram takes; the reverse inherits dsdgp_gram_grad's input_dim <= 32
 * (DSDGP_ERR_UNSUPPORTED, nothing launched).  DSDGP_ERR_UNSUPPORTED for more than 8 GB of scratch; DSDGP_ERR_BAD_ARG for M, n, DO out of
 * range, a NULL input, or a scratch block that is too small.  Asynchronous up to the read of the Cholesky status. */
int dsdgp_sparse_conditional_scratch_bytes(int64_t n, int32_t M, int32_t D, int32_t DO, int32_t reverse, int64_t* bytes);
int dsdgp_sparse_conditional(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* X, int64_t n,
                             const double* q_mu, int32_t DO, int32_t white, double jitter, void* scratch, int64_t scratch_bytes,
                             double* mean, double* var, int* info);
int dsdgp_sparse_conditional_grad(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* X, int64_t n,
                                  const double* q_mu, int32_t DO, int32_t white, double jitter, const double* gm, const double* gv,
                                  void* scratch, int64_t scratch_bytes, double* d_q_mu, double* d_Z, double* d_X, double* d_kern,
                                  int* info);

/* A stack of sparse sampled layers: DGP_Base(X, Y, likelihood, [SGPMC_Layer, ...], minibatch_size, num_samples) of the reference
 * (dgp.py:42-98 over layers.py:249-260) — dsdgp_sparse_conditional at every depth, a draw between the layers (sample_from_conditional,
 * layers.py:76-119; utils.py:40-41), the last layer not sampled (dgp.py:78-90) — its log density and the reverse pass tf.gradients builds
 * through it (csrc/sgpmc_stack.hip).  Rows r = s n + i, R = S n, as dsdgp_model_propagate.  Layer l, with input Xin (R x D_l; layer 0: X
 * repeated S times), D_l = kern.input_dim, p = input_prop_dim:
 *   Fmean = mean + m(Xin),  m = Zero, Identity (D_l = DO) or a FIXED Linear Xin A + b (mean_A (D_l x DO), mean_b (DO) or NULL: device);
 *   F = [Xin[:, :p] | Fmean + z sqrt(var + jitter)] (R x (p + DO)) = the next layer's input, so D_{l+1} = p + DO;
 *   the last layer: input_prop_dim = 0, DO = lik_width (MultiClass: the class count), no draw; its F is its Fmean.
 * Z (M x D_l), q_mu (M x DO): device.  lik_kind = any DSDGP_LIK_*, lik_p0 / lik_p1 as for dsdgp_eval_mixture. */
typedef struct {
  dsdgp_kernel kern;
  const double* Z;
  const double* q_mu;
  const double* mean_A;
  const double* mean_b;
  int32_t M, DO, white, mean_kind, input_prop_dim, reserved;
} dsdgp_stack_layer;
typedef struct {
  int32_t L, lik_kind, lik_width, reserved;
  double lik_p0, lik_p1, jitter;
  dsdgp_stack_layer layers[DSDGP_MAX_LAYERS];
} dsdgp_stack_desc;
int dsdgp_sizeof_stack_desc(void);
/* SCRATCH: everything that lives from one composed call to the next is in a block the CALLER holds (device, 256-byte aligned) of at least
 * dsdgp_stack_scratch_bytes(desc, n, S, reverse) bytes (reverse != 0: for dsdgp_stack_logdensity with a gradient); its carve-up and every
 * summation order follow from the shapes alone (csrc/sgpmc_stack_plan.hpp): no floating-point atomics, the same call gives the same bits.
 * dsdgp_stack_propagate: DGP_Base.propagate, full_cov = False (dgp.py:61-76).  zs: host array of L device pointers (R x DO_l each), or NULL
 *   / NULL entries: layer l's draws are dsdgp_randn(seed, stream = l, R DO_l); zs[L - 1] is never read.  F_out / mean_out / var_out: host
 *   arrays of L device pointers — F (R x (p + DO_l)), Fmean (R x DO_l), var (R: ONE column) — or NULL / NULL entries.
 * dsdgp_stack_logdensity: DGP_Base._build_likelihood (dgp.py:92-98) without KL terms plus the priors of layers.py:257.  Y (n x lik_width;
 *   MultiClass: n x 1 labels).  out (device, 4 doubles): [log density, data_scale / S * sum E_q log p(y | f), sum_l (-1/2 sum q_mu_l^2 -
 *   1/2 M_l DO_l log 2 pi), potrf info = 0].  grad (device, or NULL): OVERWRITTEN with the gradient of out[0] in the CONSTRAINED parameters,
 *   flat: per layer d_Z (M x D_l), d_q_mu (M x DO), d_kern (2 + (ard ? D_l : 1): variance, lengthscales, the diagonal add, as
 *   dsdgp_sparse_conditional_grad), then ONE entry for the likelihood's parameter (+0 where it has none).  The reverse pass repeats each
 *   layer's factorisation and solves (dsdgp_sparse_conditional_grad does).
 * info (host, may be NULL): the Cholesky status of the first layer whose Ku is not positive definite; every layer is factorised before
 * anything else runs, so a failure in ANY layer returns DSDGP_ERR_NOT_SPD and writes no output.  M <= 2048; the reverse inherits
 * input_dim <= 32 for every layer (DSDGP_ERR_UNSUPPORTED, nothing launched); DSDGP_ERR_UNSUPPORTED for more than 8 GB of scratch;
 * DSDGP_ERR_BAD_ARG for shapes that do not chain, a NULL input or a scratch block that is too small. */
int dsdgp_stack_scratch_bytes(const dsdgp_stack_desc* desc, int64_t n, int32_t S, int32_t reverse, int64_t* bytes);
int dsdgp_stack_propagate(dsdgp_ctx* ctx, const dsdgp_stack_desc* desc, const double* X, int64_t n, int32_t S, const double* const* zs,
                          uint64_t seed, void* scratch, int64_t scratch_bytes, double* const* F_out, double* const* mean_out,
                          double* const* var_out, int* info);
int dsdgp_stack_logdensity(dsdgp_ctx* ctx, const dsdgp_stack_desc* desc, const double* X, const double* Y, int64_t n, int32_t S,
                           const double* const* zs, uint64_t seed, double data_scale, void* scratch, int64_t scratch_bytes, double* out,
                           double* grad, int* info);
/* The hop between two layers of the stack and its reverse as calls of their own (sample_from_conditional, layers.py:76-119, and
 * utils.py:40-41; the launches the composed calls make, on the caller's arrays).  cm (R x DO), var (R), Xin (R x D_in), z (R x DO):
 *   Fmean (R x DO, or NULL) = cm + m(Xin), m by mean_kind: Zero, Identity (D_in = DO), Linear lin + b with lin = Xin A (R x DO) formed
 *   by the caller (dsdgp_gemm) and b (DO) or NULL;   F (R x (p + DO)) = [Xin[:, :p] | Fmean + z sqrt(var + jitter)].
 * Reverse, from dF (R x (p + DO)):  gm (R x DO) = dF[:, p:],  gv (R) = sum_o dF[r, p + o] z[r, o] / (2 sqrt(var_r + jitter)), ascending o
 * (a row with var + jitter = 0 has no finite gv). */
int dsdgp_stack_hop(dsdgp_ctx* ctx, const double* cm, const double* var, const double* Xin, int64_t R, int32_t D_in, int32_t mean_kind,
                    const double* lin, const double* b, int32_t p, int32_t DO, const double* z, double jitter, double* Fmean, double* F);
int dsdgp_stack_hop_bwd(dsdgp_ctx* ctx, const double* dF, int64_t R, int32_t p, int32_t DO, const double* z, const double* var,
                        double jitter, double* gm, double* gv);
/* One step of stochastic-gradient HMC (Chen, Fox and Guestrin 2014, eq. 15, noise estimate 0) over a flat vector, one launch; no
 * reference counterpart (the reference samples with gpflow.train.HMC, model_zoo.py:60-88):
 *   theta += v;  then  v = (1 - alpha) v + eta g + sqrt(2 alpha eta) xi,   g the gradient of the log density, xi N(0, 1) draws.
 * alpha = 0: plain momentum, xi is not read (and may be NULL).  DSDGP_ERR_BAD_ARG, nothing launched: alpha outside [0, 1], eta <= 0. */
int dsdgp_sghmc_step(dsdgp_ctx* ctx, int64_t count, double* theta, double* v, const double* g, const double* xi, double alpha, double eta);

/* dsdgp_pathwise_eval / dsdgp_pathwise_weights: pathwise (Matheron) draws of a sparse GP posterior FUNCTION (Wilson, Borovitskiy, Terenin,
 * Mostowsky and Deisenroth, ICML 2020).  NO reference counterpart: the reference draws rows independently (layers.py:76-119) or jointly
 * through an n x n factor (utils.py:43-51); a draw here is one function, evaluated at any inputs in any number of calls (csrc/pathwise.hip).
 * Layer with k = s2 kappa(. / l) (RBF or Matern52, scalar or ARD l, with or without a White part), inducing inputs Z (M x D):
 *   Omega (D x L): the frequencies of a random Fourier basis of kappa, ALREADY divided by l row by row;  origin c (D);
 *   theta_j(x) = sum_d (x_d - c_d) Omega_dj                   (the difference is formed first: data at an offset loses nothing)
 *   f0(x)_o    = sqrt(s2 / L) sum_j [Wc_jo cos theta_j(x) + Ws_jo sin theta_j(x)],   Wc, Ws ~ N(0, 1):  Var f0(x) = s2 exactly
 *   Ku = K(Z, Z) + (White variance + jitter) I,  Lu = chol(Ku),   u_o = q_mu_o + q_sqrt_o eps_o  (white != 0: Lu (q_mu_o + q_sqrt_o eps_o)),
 *   v = Ku^-1 (u - f0(Z))   (M x DO per draw),      f(x)_o = f0(x)_o + sum_m k(x, z_m) v_mo + add(x)_o.
 * The White part enters Ku only: f is a draw of the function WITHOUT its white component.
 * dsdgp_pathwise_eval — one launch for S draws of n rows each; every pointer a device pointer, row-major float64:
 *   X: rows of stride D = kern.input_dim; draw s reads X + s x_stride, x_stride = 0 (the same n rows for every draw) or n D;
 *   Omega (D x L, row stride L); origin (D); Wc, Ws (S x L x DO); Z (M x D); V (S x M x DO); M = 0: the prior part f0 alone, Z and V unread;
 *   add (or NULL): entry (s, i, o) at add[s add_stride + i ld_add + o], ld_add >= DO — the mean function: Identity is X itself (ld_add = D,
 *     add_stride = x_stride), Linear X A + b formed by the caller (dsdgp_gemm), Zero NULL;
 *   out: entry (s, i, o) at out[(s n + i) ld_out + o], ld_out >= DO: rows r = s n + i as dsdgp_model_propagate.  Nothing else is written.
 *   kern.lengthscales scale the distances of k(x, z); kern.variance is s2.
 * theta tiles run on the fp64 MFMA pipe (k over D, any D >= 1), sine and cosine per element, the contraction with [Wc; Ws] and the
 * K(x, Z) V term tile by tile from LDS-staged chunks; no n x L or n x M array reaches memory.  |theta| < 4096 takes a two-constant
 * reduction by pi / 2; at and above it the device library's routine: correct for every finite argument.  A NaN or infinite input row
 * gives NaN in that row's outputs only.  No atomics; the summation order of an entry follows from (L, M, D, DO) alone: the same call gives
 * the same bits, and a call on any sub-range of the rows of any one draw gives the bits those rows have in the full call.
 * Limits: L <= 65536, M <= 2048, S <= 65535, n S < 2^31, DO >= 1 (chunks of 16) — DSDGP_ERR_UNSUPPORTED beyond them and for any other
 * kernel kind; DSDGP_ERR_BAD_ARG for a NULL input, n, S, L, DO < 1, ld_out or ld_add < DO, any other x_stride; nothing is launched then.
 * dsdgp_pathwise_weights — v for S draws: eps (S x M x DO) standard normal draws, q_mu (M x DO), q_sqrt (DO x M x M, lower triangle read) or
 *   NULL: u = q_mu (Lu q_mu with white), eps is not read then.  V (S x M x DO) is OVERWRITTEN.  Composed from dsdgp_gram (symmetric form, Z
 *   moved to its first row), dsdgp_potrf, the evaluation kernel at X = Z, M = 0, dsdgp_gemm (white) and dsdgp_trsm; those use the context's
 *   scratch, so the intermediates live in `scratch` (device, 256-byte aligned, at least dsdgp_pathwise_scratch_bytes(M, D, DO, S) bytes;
 *   csrc/pathwise_plan.hpp).  info (host, may be NULL): the Cholesky status, as dsdgp_potrf; a Ku that is not positive definite returns
 *   DSDGP_ERR_NOT_SPD and writes nothing to V.  M in 1 .. 2048; DSDGP_ERR_UNSUPPORTED for more than 8 GB of scratch; DSDGP_ERR_BAD_ARG for a
 *   NULL input or a scratch block that is too small.  Asynchronous up to the read of the Cholesky status. */
int dsdgp_pathwise_eval(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* X, int64_t n, int64_t x_stride, int32_t S,
                        const double* Omega, const double* origin, int32_t L, const double* Wc, const double* Ws, const double* Z, int32_t M,
                        const double* V, int32_t DO, const double* add, int64_t ld_add, int64_t add_stride, double* out, int64_t ld_out);
int dsdgp_pathwise_scratch_bytes(int32_t M, int32_t D, int32_t DO, int32_t S, int64_t* bytes);
int dsdgp_pathwise_weights(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* Omega, const double* origin,
                           int32_t L, const double* Wc, const double* Ws, int32_t S, const double* q_mu, const double* q_sqrt,
                           const double* eps, int32_t DO, int32_t white, double jitter, void* scratch, int64_t scratch_bytes, double* V,
                           int* info);

/* out = in + value (Gaussian.predict_mean_and_var adds the noise variance, dgp.py:116-119). */
int dsdgp_add_scalar(dsdgp_ctx* ctx, const double* in, double value, int64_t count, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DSDGP_H */
