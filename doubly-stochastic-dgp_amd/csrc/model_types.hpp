// Descriptors of the model path: host-side layer and model state, the DSDGP_FORCE table, the size policy of the blocked factorisation
// (those of the chains — Csave, d-split — are chain_policy.hpp's).  LayerDev, the job records and the split counts: plan_types.hpp /
// model_plan.hpp.  Part of the model translation unit.
#pragma once
#define NPART 32
#define PREP_BLOCKS 64      // minimum; large models take more (dsdgp_model::prep_blocks: ~2048 elements of q_sqrt per thread block pass)
#define WIDE_DIN 32   // layers with D_in above this take the GEMM form of the Ku-side Z / lengthscale adjoints

struct LayerState : PlanBufs {      // (operands and partial buffers of the weight-gradient plan: model_plan.hpp)
  dsdgp_layer_desc d;
  LayerDev dev;
  int64_t R_max;    // max output rows (s_max * n_max)
  int64_t ld_max;
  double* C;
  double *F, *mean, *var, *zbuf, *dF;
  const double *meanA, *meanb;   // Linear mean function: A (fixed device array or inside theta), bias or NULL
  int njobs;                     // weight-gradient jobs of this layer in the current plan
  int njobsA = 0, totA = 0;      // ... of which the first njobsA (tasks [0, totA)) read only the forward pass's A and the upstream adjoints
  double* Xcat;     // [X_prop | F] handed to the next layer when input propagation is on (layers.py:105-110)
  int prop;
  int red_off = 0, red_blk0 = 0;   // this layer's first entry of the reduction job list / first of its blocks (they end where the next layer's begin)
  double* bpart = nullptr;      // backward-chain d-split: partial abar tiles [row block][split][Mp * 16 + 16]
  int* bcnt = nullptr;          //   arrival counters per row block (zero between launches)
  bool big = false;    // mp_blocked(Mp): multi-workgroup blocked factorisations (linalg.hpp BigChol)
  BigChol big_k, big_ngA, big_ngT;
  GemmProblem* ng_gp;  // device: 4 natural-gradient GEMM problems (H, Sinv | Y | X)
  PotrfItem* ng_items; // device: D_out factorisation items (the index-reversed A_d)
  int ng_t1, ng_t2, ng_t3;
  // the products of THIS layer that depend on (q_mu, q_sqrt) only, as launches of their own (prepare after a natural-gradient
  // step on this layer alone: the other layers' S_d / U_d / ... are still those of the previous evaluation)
  GemmProblem* lq = nullptr;
  int lq_nf = 0, lq_tf = 0, lq_n1 = 0, lq_t1 = 0, lq_n2 = 0, lq_t2 = 0, lq_np = 0, lq_tp = 0;   // forward / U, n, KS / U U^T / P_d T_d, GS_d
  WgradJob* wj;     // weight-gradient jobs of ONE launch per layer, rebuilt when (n, S) changes: [A | B] (plan_layer, model_plan.hpp)
  int ns_big, tot_big;
  bool gemm = false;     // this layer's passes are whole-layer GEMMs (layer_gemm.hip) instead of the fused chains
};

struct dsdgp_model {
  dsdgp_ctx* ctx;
  dsdgp_model_desc desc;
  int64_t n_max;
  int s_max;
  double *theta, *grad, *adam_m, *adam_v;
  LayerState L[DSDGP_MAX_LAYERS];
  LayerDev* layers_dev;
  double* mask;
  double* lik_const;   // [0] = variance, [1] = sigmoid(raw)
  double* lik_part;    // [blocks][2]
  int lik_blocks_max;
  double *lik_dmean, *lik_dvar;
  double* scal4;       // internal copy of out
  PotrfItem* potrf_items;
  GemmProblem *gp_fwd, *gp_bwd1, *gp_bwd2, *gp_w1, *gp_w2, *gp_w3;
  GemmProblem* gp_pt;   // P_d T_d (the only KL/q_sqrt GEMM that depends on the backward pass)
  int n_pt = 0, t_pt = 0;
  hipEvent_t ev_fork, ev_prep_side, ev_z;
  hipEvent_t ev_kinv;           // side stream, behind the forward-side parameter products (Ku^-1 ...): all the fused last-layer launch needs of them
  bool kinv_pending = false;
  int32_t* gemm_order = nullptr;   // device pool of the longest-processing-time tile lists of the grouped M x M launches (gemm_plan_lpt)
  int64_t gemm_order_cap = 0, gemm_order_used = 0;
  GemmLayerWs gws{};           // scratch of the GEMM-formulated layers (one set per model: the layers run one after the other)
  ParamState ps;               // what the device buffers were computed from: written by its transitions only (prepare_plan.hpp)
  int grad_first = 0;          // dsdgp_model_set_grad_first_layer: reverse mode stops below this layer
  bool grad_q_only = false;    // dsdgp_model_set_grad_q_only: only the (q_mu, q_sqrt) entries of the layers >= grad_first are wanted
  bool side_pending = false;   // parameter-only work (Ku^-1, S_d, KL, U, UU) still running on the side stream
  int n_fwd, n_bwd1, n_bwd2, t_fwd, t_bwd1, t_bwd2, n_w, t_w1, t_w2, t_w3;
  const double* sample_w = nullptr;   // DGP_Quad quadrature weights (borrowed), NULL = Monte-Carlo mean
  int sample_w_S = 0;
  GemmProblem* gp_wz;   // wm [Z | 1] of the layers with D_in > WIDE_DIN
  int n_wz = 0, t_wz = 0, kuu_blocks = 32, asm_blocks = 64, prep_blocks = PREP_BLOCKS;
  bool uniform_big = false;     // all layers share M and mp_blocked(Mp): ONE batched multi-workgroup Cholesky for all layers
  BigChol big_all;
  bool need_hyp_part = false;   // some layer does not fold its Ku-side hyper-parameter partials into k_asm_kbar
  bool tail_ok = false;         // non-white, every D_in <= WIDE_DIN: gradient assembly in k_asm_rows + k_tail (one wave per inducing row)
  struct { int on; double lr_t, b1, b2, eps; } fuse_adam = {0, 0, 0, 0, 0};   // dsdgp_model_train_step: Adam applied inside k_tail
  int mp_max_all = 0, m_max_all = 0;
  // data-parallel buckets (dsdgp_model_set_bucket_callback): one per layer in reverse order, then the likelihood / result scalars
  dsdgp_bucket_fn bucket_fn = nullptr;
  void* bucket_user = nullptr;
  double *Xmb = nullptr, *Ymb = nullptr;   // gathered minibatch of dsdgp_model_train_step_minibatch (n_max x D_in of layer 0 / x DY)
  bool head_ok = false;         // every layer has Mp <= 128 and D_in <= 16: parameter transforms, Ku, its factorisation and inverse
                                // factor (and the inner layers' N(0,1) draws) in ONE launch (k_head, head_impl.hpp)
  FwdRecord<LayerFwdArgs> fwd;  // what the reverse pass reads of the last forward pass: written by its transitions only (forward_plan.hpp)
  // arguments of the pending k_finalize (value + likelihood-variance gradient): launched on the side stream beside the
  // backward chain when streams overlap, otherwise on the main stream after it
  struct { int nblocks; double w, kl_weight; int with_grad; double* out; bool done; } fin;
  RedJob* rjobs;       // device: split reductions of every layer, rebuilt when (n, S) changes
  int rjobs_cap, n_red, red_blocks;
  size_t red_lds = 0;
  int64_t plan_n;
  int plan_S;
  // side stream: the weight-gradient products of layer l overlap the backward chain of layer l-1 (disjoint buffers)
  hipStream_t side;
  hipEvent_t ev_bwd[DSDGP_MAX_LAYERS];
  hipEvent_t ev_side;
  bool overlap;
  // DSDGP_FORCE="key=value,...": test hooks that force the large-launch variants onto small, oracle-checkable shapes (read when
  // the model is created).  save_c: Csave backward chain 0 never / 1 for Mp > 256 / 2 every size with an instance (thresholds
  // cs_min_blocks, cs_min_dout); alg_g: algebraic dl/dKu assembly -1 heuristic / 0 never / 1 always; bwd_split: d-split of the
  // backward chain 0 off / 1 from Mp = 512 / 2 everywhere; pipe_tail: per-layer reduction + P_d T_d products behind each layer's
  // weight-gradient products 0 / 1; head / tail / adj_fuse / lik_fuse = 0: the unfused launches (parity tests of the fusions);
  // ext_ev = 0: plain event record behind the head launch; red_ahead = 0: one split-K reduction after the stream join;
  // white_fwd = 0: forward-only evaluations in plain coordinates; wg_group: grouped P_d weight-gradient tasks 0 never / 1 default / 2 every D_out.  last_fuse = 0: the last layer of a training step as its two chains
  // instead of the fused launch (layer_last.hip); last_min_blocks: fewest row blocks for which the fused launch is taken.  gemm_mp: smallest padded inducing count whose layers take the
  // GEMM-formulated passes (layer_gemm.hip) instead of the fused chains, 0 = never (parity tests force it onto small shapes).
  struct Force { int save_c = 1, cs_min_blocks = 160, cs_min_dout = 3, cs_max_dout = 1 << 20, wg_defer = -1, alg_g = -1, bwd_split = 1, pipe_tail = 0, head = 1, tail = 1, adj_fuse = 1, ext_ev = 1, lik_fuse = 1, red_ahead = 1, white_fwd = 1, gemm_mp = 512, last_fuse = 1, last_min_blocks = 1, asm_pre = 1, overlap_min = 1 << 18, wg_red = 1, wg_group = 1; } force;
};
static void parse_force(dsdgp_model* m) {
  using F = dsdgp_model::Force;
  static const struct { const char* name; int F::*field; } keys[] = {
      {"save_c", &F::save_c}, {"cs_min_blocks", &F::cs_min_blocks}, {"cs_min_dout", &F::cs_min_dout}, {"cs_max_dout", &F::cs_max_dout},
      {"wg_defer", &F::wg_defer}, {"alg_g", &F::alg_g}, {"bwd_split", &F::bwd_split}, {"red_ahead", &F::red_ahead},
      {"white_fwd", &F::white_fwd}, {"pipe_tail", &F::pipe_tail}, {"head", &F::head}, {"tail", &F::tail}, {"adj_fuse", &F::adj_fuse},
      {"ext_ev", &F::ext_ev}, {"lik_fuse", &F::lik_fuse}, {"gemm_mp", &F::gemm_mp}, {"last_fuse", &F::last_fuse},
      {"last_min_blocks", &F::last_min_blocks}, {"asm_pre", &F::asm_pre}, {"overlap_min", &F::overlap_min}, {"wg_red", &F::wg_red},
      {"wg_group", &F::wg_group}};
  const char* e = getenv("DSDGP_FORCE");
  if (!e) return;
  const std::string str(e);
  for (size_t pos = 0; pos < str.size();) {
    size_t end = str.find(',', pos);
    if (end == std::string::npos) end = str.size();
    const std::string kv = str.substr(pos, end - pos);
    const size_t eq = kv.find('=');
    if (eq != std::string::npos)
      for (const auto& k : keys)      // (unknown keys are ignored)
        if (kv.compare(0, eq, k.name) == 0) m->force.*k.field = atoi(kv.c_str() + eq + 1);
    pos = end + 1;
  }
}

struct Bump {
  char* base;
  size_t off;
  template <class T>
  T* take(size_t count) {
    off = (size_t)round_up((int64_t)off, 256);
    T* p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};

// padded inducing count from which the multi-workgroup blocked Cholesky / inverse replaces the one-workgroup kernel (chol_plan.hpp:
// chol_route).  Layers that share M are factorised as ONE batch.
static int big_mp(bool uniform) {
  static const int nonuniform = getenv("DSDGP_BIG_MP") ? atoi(getenv("DSDGP_BIG_MP")) : CHOL_BLOCKED_MIN;      // (A/B aid)
  return uniform ? CHOL_BLOCKED_MIN : nonuniform;
}
// a model's Mp is fixed by the chain kernels (pad_M): the blocked sequence takes it from big_mp() on, as a multiple of 64
static bool mp_blocked(int Mp, bool uniform) { return chol_route(Mp, big_mp(uniform), false).kind == CHOL_BLOCKED; }
