// Launch schedule of one evaluation: prepare (Ku, factor, parameter products; main / side stream — what of them is redone is decided
// once, by prep_plan of prepare_plan.hpp, from the validity record dsdgp_model::ps), forward layers (dgp.py:61-76) — their decisions taken
// once per call by fwd_plan of forward_plan.hpp, then launches only (forward_pass, forward_layers), leaving the record dsdgp_model::fwd —
// upload of the split-K plan (ensure_plan; the arithmetic is model_plan.hpp), reverse pass — its decisions taken once (BwdSchedule,
// bwd_schedule), then launches only (backward_layers and its three endings) — ELBO / training step.  Part of the model translation unit.
#pragma once
// Side-stream overlap pays for its cross-stream events (a few microseconds each) only when the kernels are long enough:
// tiny models (cfg 1: 100 rows, M = 50: n S Mp = 6400) are launch-latency-bound and run 40 % faster on a single stream.  The threshold
// (DSDGP_FORCE overlap_min, default 2^18; 2^20 until round 6) sits below the 125- and 250-row shards of config 2's strong-scaling run
// (n S Mp = 3.2e5 / 6.4e5): overlapped they take 0.297 / 0.342 ms per data-parallel step against 0.317 / 0.368 on one stream.
static bool overlap_on(const dsdgp_model* m, int64_t n, int S) {
  const char* no = getenv("DSDGP_NO_OVERLAP");   // read per call so that a profiler can serialise the kernels
  if (!m->overlap || (no && atoi(no))) return false;
  int mp_max = 0;
  for (int l = 0; l < m->desc.L; ++l) mp_max = std::max(mp_max, (int)m->L[l].dev.Mp);
  return n * S * (int64_t)mp_max >= (int64_t)m->force.overlap_min;
}

// The four sub-lists of a layer's own grouped-GEMM problems (LayerState::lq: forward | U, n, KS | U U^T | P_d T_d, GS_d) start here
static const GemmProblem* lq_unks(const LayerState& S) { return S.lq + S.lq_nf; }
static const GemmProblem* lq_uut(const LayerState& S) { return lq_unks(S) + S.lq_n1; }
static const GemmProblem* lq_pt(const LayerState& S) { return lq_uut(S) + S.lq_n2; }

// main stream waits for the parameter-only side work of the last prepare (no-op when nothing is pending)
static int join_prep(dsdgp_model* m) {
  if (m->side_pending) {
    DS_HIP(hipStreamWaitEvent(m->ctx->stream, m->ev_prep_side, 0));
    m->side_pending = false;
  }
  return DSDGP_OK;
}

// Parameter transforms, Ku, its Cholesky / inverse factor (main stream: the forward chain needs exactly these), then the
// parameter-only rest — Ku^-1, S_d, Lu^-1 q_sqrt, KL and, for a gradient step, U_d = Ku^-1 q_sqrt_d, n = Ku^-1 q_mu and
// U_d U_d^T — which nothing needs before the backward pass / the final reduction: with `side` it runs on the side stream
// concurrently with the forward layers and the caller joins (join_prep) where it is first consumed.
// (`side` = run that part on the side stream.)  What is redone and what stays is prep_plan's decision (prepare_plan.hpp: the reuse
// rules under dsdgp_model_track_theta); here: its inputs, then the launches it names.
static_assert(DSDGP_MAX_LAYERS <= 32, "PrepIn::blocked is a 32-bit mask");
static PrepIn prep_in(const dsdgp_model* m, bool with_grad, bool side) {
  PrepIn in{with_grad, side, m->desc.L, m->desc.white != 0, m->grad_first, m->head_ok, m->uniform_big, 0u, 0, big_mp(false), m->force.ext_ev != 0};
  for (int l = 0; l < in.L; ++l) {
    in.mp_max = std::max(in.mp_max, (int)m->L[l].dev.Mp);
    if (m->L[l].big) in.blocked |= 1u << l;
  }
  return in;
}
static int launch_grad_side(dsdgp_ctx* ctx, const LayerState& Sq, hipStream_t st) {      // U_d, n, KS | U_d U_d^T of one layer
  DS_TRY(gemm_launch(ctx, lq_unks(Sq), Sq.lq_n1, Sq.lq_t1, st));
  return gemm_launch(ctx, lq_uut(Sq), Sq.lq_n2, Sq.lq_t2, st);
}
static int prepare_async(dsdgp_model* m, bool with_grad = false, bool side = false, const HeadRand* hr = nullptr,
                         const HeadGather* hg = nullptr) {
  dsdgp_ctx* ctx = m->ctx;
  const int L = m->desc.L;
  m->ps.workspace_overwritten();
  DS_TRY(join_prep(m));
  const PrepIn in = prep_in(m, with_grad, side);
  const PrepPlan p = prep_plan(m->ps, in);
  const int mp_max = in.mp_max;
  if (p.head) {
    ProfScope ps(ctx, "potrf");
    const size_t lds = head_lds_bytes(mp_max);
    static size_t lds_set = 0;     // the attribute is sticky: one driver call per size
    if (lds > lds_set) {
      DS_HIP(hipFuncSetAttribute((const void*)k_head, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      lds_set = lds;
    }
    HeadRand none{};
    const HeadRand& r = hr ? *hr : none;
    HeadGather gnone{};
    const HeadGather& gq = hg ? *hg : gnone;
    const int nprep = std::max(32, m->prep_blocks / 2);
    // fork_on_head: with a side stream the launch carries the fork event itself (hipExtLaunchKernel attaches it to the dispatch's completion signal):
    // a separate hipEventRecord puts a marker packet on this stream that the next kernel queues behind (~6 us, profiles/r03_timeline_*)
    g_dsdgp_launches.fetch_add(1, std::memory_order_relaxed);
    hipExtLaunchKernelGGL(k_head, dim3(1 + nprep + r.nblk + gq.nblk, L), dim3(HEAD_THREADS), (uint32_t)lds, ctx->stream, nullptr,
                          p.fork_on_head ? m->ev_fork : nullptr, 0, (const double*)m->theta, (const LayerDev*)m->layers_dev, m->lik_const,
                          (int64_t)m->desc.off_lik_var, lik_has_param(m->desc.lik_kind) ? 1 : 0, m->desc.jitter, nprep,
                          p.keep_kuu ? 1 : 0, m->desc.white ? 1 : 0, getenv("DSDGP_POTRF_TIMING") ? 1 : 0, r, gq);
    DS_HIP(hipGetLastError());
  } else if (p.prep_kuu) {
    DS_LAUNCH(k_prep_kuu, dim3(m->prep_blocks + (p.kuu_blocks ? m->kuu_blocks : 0), L), dim3(256), 0, ctx->stream, m->theta, m->layers_dev,
                       m->lik_const, m->desc.off_lik_var, lik_has_param(m->desc.lik_kind) ? 1 : 0, m->desc.jitter,
                       m->prep_blocks, p.keep_kuu ? 1 : 0);
    DS_HIP(hipGetLastError());
  }
  switch (p.factor) {
    case FACTOR_NONE: case FACTOR_IN_HEAD: break;
    case FACTOR_BATCHED_BLOCKED: DS_TRY(bigchol_run(ctx, m->big_all)); break;
    case FACTOR_PER_LAYER:
      for (int l = 0; l < L; ++l) {
        if (p.blocked >> l & 1) DS_TRY(bigchol_run(ctx, m->L[l].big_k));
        else DS_TRY(potrf_launch(ctx, m->potrf_items + l, 1, m->L[l].dev.Mp));
      }
      break;
    case FACTOR_ONE_WG_BATCH: DS_TRY(potrf_launch(ctx, m->potrf_items, L, mp_max)); break;
  }
  if (p.early) {
    m->ps.prepare_done(p);
    return DSDGP_OK;
  }
  hipStream_t st = ctx->stream;
  if (p.fork) {
    if (!p.fork_on_head) DS_HIP(hipEventRecord(m->ev_fork, ctx->stream));
    DS_HIP(hipStreamWaitEvent(m->side, m->ev_fork, 0));
    st = m->side;
  }
  const int klb = mp_max >= 512 ? 512 : NPART;    // M = 512 / 1024: V alone is 8..64 MB per layer — 32 workgroups were latency-bound
  if (p.fwd == REDO_LAYER) {
    LayerState& Sq = m->L[p.fwd_layer];
    DS_TRY(gemm_launch(ctx, Sq.lq, Sq.lq_nf, Sq.lq_tf, st));
    DS_LAUNCH(k_kl_part, dim3(klb, 1), dim3(256), 0, st, m->layers_dev + p.fwd_layer);
  } else if (p.fwd == REDO_ALL) {
    DS_TRY(gemm_launch(ctx, m->gp_fwd, m->n_fwd, m->t_fwd, st));
    DS_LAUNCH(k_kl_part, dim3(klb, L), dim3(256), 0, st, m->layers_dev);
  }
  DS_HIP(hipGetLastError());
  m->kinv_pending = false;
  if (p.rec_kinv) {
    // Ku^-1, S_d and Lu^-1 q_sqrt are in the launch above — everything the backward CHAINS read of the side stream's products (the
    // rest — KS_d, U_d, n, U_d U_d^T — feeds the assembly at the end of the step).  The reverse pass waits for THIS event, long since
    // signalled when the forward chains end; the whole side stream's work ends together with the last inner forward chain, and a
    // just-in-time cross-stream wait there cost ~12 us of idle main stream in front of the first launch of the reverse pass
    // (profiles/r06_timeline_step.txt).  The rest is covered by the join at the end of the reverse pass (the side stream is in order).
    DS_HIP(hipEventRecord(m->ev_kinv, m->side));
    m->kinv_pending = true;
  }
  if (p.grad == REDO_LAYER) DS_TRY(launch_grad_side(ctx, m->L[p.grad_layer], st));
  else if (p.grad == REDO_FROM) {
    for (int l = p.grad_layer; l < L; ++l) DS_TRY(launch_grad_side(ctx, m->L[l], st));
  } else if (p.grad == REDO_ALL) {
    DS_TRY(gemm_launch(ctx, m->gp_bwd1, m->n_bwd1, m->t_bwd1, st));
    DS_TRY(gemm_launch(ctx, m->gp_bwd2, m->n_bwd2, m->t_bwd2, st));
  }
  if (p.rec_prep_side) {
    DS_HIP(hipEventRecord(m->ev_prep_side, m->side));
    m->side_pending = true;
  }
  m->ps.prepare_done(p);
  return DSDGP_OK;
}
static int ensure_prepared(dsdgp_model* m) { return m->ps.prepared ? DSDGP_OK : prepare_async(m); }

static int read_info(dsdgp_model* m, int* info) {
  if (!info) return DSDGP_OK;
  *info = 0;
  if (getenv("DSDGP_POTRF_TIMING")) {   // debug aid: per-phase shader cycles of layer 0's factorisation
    double sc[12];
    hipMemcpyAsync(sc, m->L[0].dev.scal, sizeof(sc), hipMemcpyDeviceToHost, m->ctx->stream);
    hipStreamSynchronize(m->ctx->stream);
    if (m->head_ok)
      fprintf(stderr, "[head cycles] start + Z staging %.0f | Ku %.0f | first panel %.0f | block columns 1.. (+ inverse rows) %.0f | logdet + last two "
              "inverse rows %.0f || wave 0 in the loop: tile %.0f, barrier %.0f, panel %.0f, barrier %.0f\n", sc[2], sc[3], sc[4], sc[5], sc[6], sc[7],
              sc[8], sc[9], sc[10]);
    else
      fprintf(stderr, "[potrf cycles] factor %.0f inverse %.0f panel %.0f trailing %.0f logdet+writeback %.0f copyin+trtri %.0f\n", sc[2],
              sc[3], sc[4], sc[5], sc[6], sc[7]);
  }
  for (int l = 0; l < m->desc.L; ++l) {
    double sc[2];
    DS_HIP(hipMemcpyAsync(sc, m->L[l].dev.scal, sizeof(sc), hipMemcpyDeviceToHost, m->ctx->stream));
    DS_HIP(hipStreamSynchronize(m->ctx->stream));
    if (sc[1] != 0.0 && *info == 0) *info = (int)sc[1];
  }
  if (*info) {
    dsdgp_set_error("Cholesky decomposition was not successful (layer Kuu pivot %d)", *info);
    return DSDGP_ERR_NOT_SPD;
  }
  return DSDGP_OK;
}

extern "C" int dsdgp_model_prepare(dsdgp_model* m, int* info) {
  DS_CHECK_ARG(m != nullptr);
  DS_TRY(prepare_async(m));
  return read_info(m, info);
}

static int randn_async(dsdgp_ctx* ctx, uint64_t seed, uint64_t stream, int64_t count, double* out, hipStream_t st = nullptr) {
  const int nb = (int)std::min<int64_t>(2048, ceil_div((count + 1) / 2, 256));
  DS_LAUNCH(k_randn, dim3(nb > 0 ? nb : 1), dim3(256), 0, st ? st : ctx->stream, seed, stream, count, out);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// A forward pass as its entry point states it: inputs, draws (zs / zstride as dsdgp_model_propagate takes them; what they leave open is
// drawn from `seed`), optional output arrays per layer, the likelihood's targets and weight (data_scale / S) for the chain epilogue
struct FwdCall {
  const double* X;
  int64_t n;
  int S;
  const double* const* zs;
  const int64_t* zstride;
  uint64_t seed;
  double *const *Fs, *const *Fmeans, *const *Fvars;
  const double* lik_Y;
  double lik_w;
};
// minibatch to gather before the evaluation (dsdgp_model_train_step_minibatch): rows idx[0..n) of the resident data
struct GatherSrc {
  const double *Xs, *Ys;
  const int64_t* idx;
};
// The call and the model as fwd_plan takes them (forward_plan.hpp).  prepare: the call runs a prepare of its own; save: for a reverse pass
static FwdIn fwd_in(const dsdgp_model* m, const FwdCall& c, bool prepare, bool save, bool need_last_F, bool lik_target) {
  static const bool timing = getenv("DSDGP_FWD_TIMING") || getenv("DSDGP_BWD_TIMING");
  const dsdgp_model::Force& f = m->force;
  FwdIn in{};
  in.n = c.n; in.S = c.S;
  in.prepare = prepare; in.save = in.with_grad = save; in.need_last_F = need_last_F; in.lik_target = lik_target; in.sample_w = m->sample_w != nullptr;
  in.L = m->desc.L; in.white = m->desc.white != 0;
  in.lik_elementwise = lik_family(m->desc.lik_kind) != LIKF_NONE; in.lik_gaussian = m->desc.lik_kind == DSDGP_LIK_GAUSSIAN;
  in.grad_first = m->grad_first; in.grad_q_only = m->grad_q_only; in.head_ok = m->head_ok; in.overlap = overlap_on(m, c.n, c.S); in.timing = timing;
  for (int l = 0; l < in.L; ++l) {
    const LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    if (c.zs && c.zs[l]) in.caller_z |= 1u << l;
    in.layer[l] = FwdIn::Layer{v.Mp, v.M, v.D_in, v.D_out, v.kern_kind, St.d.mean_kind, St.prop, St.gemm, v.alg_g != 0, v.need_tpt != 0, St.C != nullptr,
                               St.bpart != nullptr};
  }
  in.force = {f.white_fwd, f.cs_min_blocks, f.cs_min_dout, f.cs_max_dout, f.last_fuse, f.last_min_blocks, f.bwd_split, f.lik_fuse};
  return in;
}

// dgp.py:61-76 propagate.  The decisions are fwd_plan's; here: every layer's argument block as the plan says, its launch, and the record
// of the pass for the reverse pass (dsdgp_model::fwd)
static int forward_layers(dsdgp_model* m, const FwdCall& c, const FwdIn& in, const FwdPlan& p) {
  dsdgp_ctx* ctx = m->ctx;
  const int L = m->desc.L;
  m->ps.workspace_overwritten();
  if (p.join_prep_first) DS_TRY(join_prep(m));
  const double* Xin = c.X;
  FwdUsed used[DSDGP_MAX_LAYERS];
  LayerFwdArgs a{};
  for (int l = 0; l < L; ++l) {
    LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    const FwdPlan::Layer& y = p.layer[l];
    a = LayerFwdArgs{};
    a.X = Xin; a.Rin = y.Rin; a.rep = y.rep;
    a.D_in = v.D_in; a.D_out = v.D_out; a.M = v.M;
    a.Zp = v.Zp; a.Zs = v.Zs; a.hyp = v.hyp; a.LinvT = v.LinvT; a.Linv = v.Linv; a.Tp = v.Tp; a.TpT = v.TpT; a.qmu = v.qmu;
    if (y.whitened) { a.Tp = v.V; a.qmu = v.nL; a.qmu_ld = v.DP4; }
    a.mean_kind = St.d.mean_kind; a.mean_A = St.meanA; a.mean_b = St.meanb;
    a.jitter = m->desc.jitter;
    a.n_inner = c.n;
    if (y.draw == DRAW_CALLER) {
      a.z = c.zs[l];
      a.zs_s = c.zstride[3 * l]; a.zs_n = c.zstride[3 * l + 1]; a.zs_d = c.zstride[3 * l + 2];
    } else if (y.draw != DRAW_NONE) {
      if (y.draw == DRAW_HERE) DS_TRY(randn_async(ctx, c.seed, (uint64_t)l, (int64_t)c.S * c.n * v.D_out, St.zbuf));
      a.z = St.zbuf;
      a.zs_s = c.n * v.D_out; a.zs_n = v.D_out; a.zs_d = 1;
    }
    a.F = y.want_F ? ((c.Fs && c.Fs[l]) ? c.Fs[l] : St.F) : nullptr;
    a.mean = (c.Fmeans && c.Fmeans[l]) ? c.Fmeans[l] : St.mean;
    a.var = (c.Fvars && c.Fvars[l]) ? c.Fvars[l] : St.var;
    a.ldA = y.ld;
    a.Asave = y.save_A ? St.A : nullptr; a.Csave = y.save_C ? St.C : nullptr; a.XT1 = y.save_XT1 ? St.XT1 : nullptr;
    a.d_split = y.d_split;
    if (y.lik_epilogue) {
      a.lik_Y = c.lik_Y; a.lik_const = m->lik_const; a.lik_w = c.lik_w; a.lik_part = m->lik_part;
      a.lik_MB = St.MB; a.lik_VB = St.VB; a.lik_ld = y.ld;
    }
    switch (y.launch) {
      case LAUNCH_WITH_REVERSE: break;      // backward_layers launches it together with this layer's reverse pass
      case LAUNCH_GEMM: DS_TRY(layer_fwd_gemm_launch(ctx, a, v.Mp, v.kern_kind, m->desc.white ? 1 : 0, m->gws)); break;
      case LAUNCH_CHAIN: DS_TRY(layer_fwd_sm_launch(ctx, a, v.Mp, v.kern_kind, m->desc.white || y.whitened)); break;
    }
    used[l] = FwdUsed{a.X, a.z, a.zs_s, a.zs_n, a.zs_d};
    if (y.concat) {
      const int64_t R = (int64_t)c.S * c.n, cnt = R * (v.D_out + St.prop);
      DS_LAUNCH(k_concat_prop, dim3((int)std::min<int64_t>(4096, ceil_div(cnt, 256))), dim3(256), 0, ctx->stream, Xin, y.Rin,
                         v.D_in, St.prop, a.F, v.D_out, R, St.Xcat);
      DS_HIP(hipGetLastError());
      Xin = St.Xcat;
    } else {
      Xin = a.F;
    }
  }
  m->fwd.forward_done(in, p, used, p.layer[L - 1].launch == LAUNCH_WITH_REVERSE ? &a : nullptr);
  return DSDGP_OK;
}

// The N(0,1) draws of the inner layers that no explicit zs covers (DRAW_READY), ahead of the factorisation they do not depend on: in
// spare block columns of the fused head launch (head_rand: the block prepare_async hands it), else — overlapped schedule — on the side
// stream while Ku is factorised (inner_draws: the caller waits for ev_z behind prepare_async).  Neither: forward_layers draws them itself.
static HeadRand head_rand(const dsdgp_model* m, const FwdCall& c, const FwdPlan& p) {
  HeadRand hr{};
  hr.seed = c.seed; hr.nblk = p.head_nblk;
  for (int l = 0; l < m->desc.L; ++l)
    if (p.layer[l].draw == DRAW_READY) {
      hr.out[l] = m->L[l].zbuf;
      hr.count[l] = (int64_t)c.S * c.n * m->L[l].dev.D_out;
    }
  return hr;
}
static int inner_draws(dsdgp_model* m, const FwdCall& c, const FwdPlan& p) {
  DS_HIP(hipEventRecord(m->ev_fork, m->ctx->stream));     // after the previous step's readers of zbuf
  DS_HIP(hipStreamWaitEvent(m->side, m->ev_fork, 0));
  for (int l = 0; l < m->desc.L; ++l)
    if (p.layer[l].draw == DRAW_READY) DS_TRY(randn_async(m->ctx, c.seed, (uint64_t)l, (int64_t)c.S * c.n * m->L[l].dev.D_out, m->L[l].zbuf, m->side));
  if (p.draws_ahead) DS_HIP(hipEventRecord(m->ev_z, m->side));
  return DSDGP_OK;
}
// The front of every forward pass: the plan; then, where the call prepares (an evaluation, a saved pass), the draws where the plan places
// them, the minibatch gather, prepare, the wait for the side stream's draws — a call that does not (propagate, the mixtures) only makes
// sure that the model is prepared; then the chains.  *plan: what was decided, for the caller's likelihood launches.
static int forward_pass(dsdgp_model* m, const FwdCall& c, const FwdIn& in, const GatherSrc* gs = nullptr, FwdPlan* plan = nullptr) {
  DS_CHECK_ARG(c.n > 0 && c.n <= m->n_max && c.S > 0 && c.S <= m->s_max);
  const FwdPlan p = fwd_plan(in);
  if (in.prepare) {
    const bool ahead_in_head = p.draws == DRAWS_HEAD && p.draws_ahead;
    const HeadRand hr = ahead_in_head ? head_rand(m, c, p) : HeadRand{};
    if (p.draws == DRAWS_SIDE) DS_TRY(inner_draws(m, c, p));
    HeadGather hg{};
    if (gs) {
      const int dx = m->desc.layers[0].D_in, dy = (m->desc.lik_kind == DSDGP_LIK_MULTICLASS) ? 1 : m->desc.layers[in.L - 1].D_out;
      if (m->head_ok) {
        hg = HeadGather{gs->Xs, gs->Ys, gs->idx, m->Xmb, m->Ymb, c.n, dx, dy, (int)std::min<int64_t>(16, ceil_div(c.n * (dx + dy), 2 * HEAD_THREADS))};
      } else {
        DS_TRY(dsdgp_gather_rows2(m->ctx, gs->Xs, dx, m->Xmb, gs->Ys, dy, m->Ymb, gs->idx, c.n, 0));
      }
    }
    DS_TRY(prepare_async(m, in.with_grad, in.overlap, ahead_in_head ? &hr : nullptr, (gs && m->head_ok) ? &hg : nullptr));
    if (p.draws == DRAWS_SIDE && p.draws_ahead) DS_HIP(hipStreamWaitEvent(m->ctx->stream, m->ev_z, 0));
  } else {
    DS_TRY(ensure_prepared(m));
  }
  if (plan) *plan = p;
  return forward_layers(m, c, in, p);
}

extern "C" int dsdgp_model_propagate(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs,
                                     const int64_t* zstride, uint64_t seed, double* const* Fs, double* const* Fmeans,
                                     double* const* Fvars) {
  DS_CHECK_ARG(m && X);
  DS_CHECK_ARG(!zs || zstride);
  const FwdCall c{X, n, S, zs, zstride, seed, Fs, Fmeans, Fvars, nullptr, 0.0};
  return forward_pass(m, c, fwd_in(m, c, false, false, true, false));
}

// The front that the three mixture entries below share: their refusals, then the forward pass of dsdgp_model_propagate with only the
// last layer's mean and variance wanted (they stay in the workspace; *last is that layer).  The reduction follows on the same stream and
// reads the likelihood's positive parameter from the model's own device copy: nothing goes through the host.
static int mixture_forward(const char* who, dsdgp_model* m, const double* X, int64_t n, int S, const double* const* zs,
                           const int64_t* zstride, uint64_t seed, bool needs_gaussian, const LayerState** last) {
  DS_CHECK_ARG(!zs || zstride);
  if (m->sample_w) {
    dsdgp_set_error("%s: quadrature sample weights are set (dsdgp_model_set_sample_weights); the mixture is an unweighted mean", who);
    return DSDGP_ERR_UNSUPPORTED;
  }
  if (needs_gaussian && m->desc.lik_kind != DSDGP_LIK_GAUSSIAN) {
    dsdgp_set_error("%s: the predictive y of likelihood kind %d is not a Gaussian mixture; only the latent f (level 0) is covered", who,
                    m->desc.lik_kind);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const FwdCall c{X, n, S, zs, zstride, seed, nullptr, nullptr, nullptr, nullptr, 0.0};
  DS_TRY(forward_pass(m, c, fwd_in(m, c, false, false, true, false)));
  *last = &m->L[m->desc.L - 1];
  return DSDGP_OK;
}

// Held-out evaluation (demos/run_regression.py:108-123 on dgp.py:116-126): the mixture reduction of evaluate.hip
extern "C" int dsdgp_model_evaluate(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                                    const int64_t* zstride, uint64_t seed, double* rows_out, double* acc, int accumulate) {
  DS_CHECK_ARG(m && X && Y && acc);
  const LayerState* last;
  DS_TRY(mixture_forward("dsdgp_model_evaluate", m, X, n, S, zs, zstride, seed, false, &last));
  const int kind = m->desc.lik_kind;
  DS_CHECK_ARG(kind != DSDGP_LIK_MULTICLASS || last->dev.D_out == m->desc.num_classes);
  return eval_mixture_launch(m->ctx, kind, 1.0, m->desc.lik_aux, lik_has_param(kind) ? m->lik_const : nullptr, last->mean, last->var, Y, n,
                             S, last->dev.D_out, rows_out, acc, accumulate);
}

// Calibration of the predictive mixture: the quantile / PIT + CRPS kernel of calibration.hip
extern "C" int dsdgp_model_quantiles(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs,
                                     const int64_t* zstride, uint64_t seed, int32_t level, const double* probs, int32_t P,
                                     double* q_out) {
  DS_CHECK_ARG(m && X && probs && q_out);
  DS_CHECK_ARG(!zs || zstride);      // (here as well: a bad call keeps meeting this check before the one on level)
  DS_CHECK_ARG(level == 0 || level == 1);
  const LayerState* last;
  DS_TRY(mixture_forward("dsdgp_model_quantiles", m, X, n, S, zs, zstride, seed, level == 1, &last));
  return mixture_quantiles_launch(m->ctx, last->mean, last->var, 0.0, level == 1 ? m->lik_const : nullptr, n, S, last->dev.D_out, probs, P,
                                  q_out);
}
extern "C" int dsdgp_model_calibration(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                                       const int64_t* zstride, uint64_t seed, const double* probs, int32_t P, double* rows_out,
                                       double* acc, int accumulate) {
  DS_CHECK_ARG(m && X && Y && probs && acc);
  const LayerState* last;
  DS_TRY(mixture_forward("dsdgp_model_calibration", m, X, n, S, zs, zstride, seed, true, &last));
  return mixture_calibration_launch(m->ctx, last->mean, last->var, 0.0, m->lik_const, Y, n, S, last->dev.D_out, probs, P, rows_out, acc,
                                    accumulate);
}

// Classification report of the predictive mixture (MultiClass / Bernoulli): the probability and report kernels of classification.hip
extern "C" int dsdgp_model_classification(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                                          const int64_t* zstride, uint64_t seed, int32_t bins, double* probs_out, double* rows_out,
                                          double* acc, int accumulate) {
  DS_CHECK_ARG(m && X && Y && acc);
  const int kind = m->desc.lik_kind;
  if (kind != DSDGP_LIK_MULTICLASS && kind != DSDGP_LIK_BERNOULLI) {
    dsdgp_set_error("dsdgp_model_classification: likelihood kind %d has no classes; MultiClass and Bernoulli are covered", kind);
    return DSDGP_ERR_UNSUPPORTED;
  }
  const LayerState* last;
  DS_TRY(mixture_forward("dsdgp_model_classification", m, X, n, S, zs, zstride, seed, false, &last));
  DS_CHECK_ARG(kind != DSDGP_LIK_MULTICLASS || last->dev.D_out == m->desc.num_classes);
  return mixture_classification_launch(m->ctx, kind, last->mean, last->var, Y, n, S, last->dev.D_out, bins, probs_out, rows_out, acc,
                                       accumulate);
}

// (re)build the split-K job lists for minibatch shape (n, S); uploaded once, reused by every step of that shape.  The arithmetic is
// model_plan.hpp's (pure host code, tests/test_plan_cpu.py); here: capacity checks, clearing, uploads, the record in St / m.
static int ensure_plan(dsdgp_model* m, int64_t n, int S) {
  if (m->plan_n == n && m->plan_S == S) return DSDGP_OK;
  dsdgp_ctx* ctx = m->ctx;
  const int L = m->desc.L, overlap = overlap_on(m, n, S);
  std::vector<RedJob> red;
  PlanOut P;
  for (int l = 0; l < L; ++l) {
    LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    const int64_t ld = round_up((l == 0) ? n : (int64_t)S * n, 16);
    const int hyp_parts = St.gemm ? layer_gemm_hyp_parts(ld, v.Mp) : (int)sm_hyp_parts(ld, v.Mp, v.D_in);
    plan_layer(PlanIn{&v, &St, ld, hyp_parts, m->force.wg_red, m->force.wg_group, overlap}, P);
    if (P.ticks > St.cap.ticks) {
      dsdgp_set_error("internal: weight-gradient ticket list overflow (%d > %d)", P.ticks, St.cap.ticks);
      return DSDGP_ERR_WORKSPACE;
    }
    if ((int)P.jobs.size() > St.cap.jobs) {
      dsdgp_set_error("internal: weight-gradient job list overflow (%d jobs > %d slots of wj)", (int)P.jobs.size(), St.cap.jobs);
      return DSDGP_ERR_WORKSPACE;
    }
    St.njobs = (int)P.jobs.size(); St.njobsA = P.njobsA; St.totA = P.totA; St.tot_big = P.tot; St.ns_big = P.ns;
    St.red_off = (int)red.size();
    red.insert(red.end(), P.red.begin(), P.red.end());
    DS_HIP(hipMemsetAsync(St.wtick, 0, (size_t)St.cap.ticks * sizeof(int32_t), ctx->stream));
    // diagonal tiles fill only their first ns_diag partial slots: the rest must read as zero under the new plan
    DS_HIP(hipMemsetAsync(St.part_big, 0, St.cap.part_big * sizeof(double), ctx->stream));
    DS_HIP(hipMemcpyAsync(St.wj, P.jobs.data(), P.jobs.size() * sizeof(WgradJob), hipMemcpyHostToDevice, ctx->stream));
    DS_HIP(hipStreamSynchronize(ctx->stream));
  }
  const RedPlan rp = plan_reductions(red);
  for (int l = 0; l < L; ++l) m->L[l].red_blk0 = red[m->L[l].red_off].blk_start;      // (every layer has its hyper-parameter job)
  if ((int)red.size() > m->rjobs_cap) {
    dsdgp_set_error("internal: reduction job list overflow");
    return DSDGP_ERR_WORKSPACE;
  }
  DS_HIP(hipMemcpyAsync(m->rjobs, red.data(), red.size() * sizeof(RedJob), hipMemcpyHostToDevice, ctx->stream));
  DS_HIP(hipStreamSynchronize(ctx->stream));
  m->n_red = (int)red.size(); m->red_blocks = rp.blocks;
  m->red_lds = rp.any64 ? 64 * 65 * sizeof(double) : 0;      // dynamic LDS of k_reduce_grouped: the 64 x 64 copy-and-mirror tile
  m->plan_n = n; m->plan_S = S;
  return DSDGP_OK;
}

// layer l's parameters are one segment of theta: [off_Z, next layer's off_Z); the last ends at the likelihood's parameter or the vector's end
static int64_t theta_segment_lo(const dsdgp_model* m, int l) {
  return l < m->desc.L ? m->L[l].d.off_Z : (lik_has_param(m->desc.lik_kind) ? m->desc.off_lik_var : m->desc.n_theta);
}
// offset of the likelihood's positive parameter in theta / grad, -1: it has none
static int64_t lik_var_offset(const dsdgp_model* m) { return lik_has_param(m->desc.lik_kind) ? m->desc.off_lik_var : (int64_t)-1; }
static FinArgs fin_args(const dsdgp_model* m) {
  return FinArgs{m->lik_part, m->fin.nblocks, m->fin.w, m->fin.kl_weight, m->lik_const, lik_var_offset(m), m->fin.out, m->desc.L, 1};
}

static int launch_finalize(dsdgp_model* m, hipStream_t st) {
  DS_LAUNCH(k_finalize, dim3(1), dim3(256), 0, st, m->layers_dev, m->desc.L, m->lik_part, m->fin.nblocks, m->fin.w,
                     m->fin.kl_weight, m->lik_const, m->grad, lik_var_offset(m), m->fin.with_grad, m->fin.out);
  DS_HIP(hipGetLastError());
  m->fin.done = true;
  return DSDGP_OK;
}

// The schedule of one reverse pass: every decision, taken once before the first launch (bwd_schedule; on the caller's stack).
// Who writes a layer's transposed upstream adjoints MB / VB (+ [X^T ; 1]): the producer where one exists — the likelihood kernel
// for the last layer, the next layer's backward chain for inner layers; for a first layer below others this layer's own backward
// chain in its prologue (LayerBwdArgs::up_dF); else (first layer: S output rows per input row; MultiClass) k_adj_prep
enum AdjFrom : uint8_t { ADJ_PRODUCER, ADJ_PROLOGUE, ADJ_PREP };
// Where a layer's weight-gradient products go: main stream behind its chain, side stream behind an event at the end of its chain,
// or main stream behind the lowest layer's products (defer_upper)
enum ProductsAt : uint8_t { PROD_MAIN, PROD_SIDE, PROD_DEFERRED };
struct BwdSchedule {
  int gfirst; bool overlap, bucketed, pipelined, kinv_only, q_only, defer_upper, red_ahead;
  struct Layer { AdjFrom adj; bool chain; int d_split; ProductsAt products; } layer[DSDGP_MAX_LAYERS];      // entries [gfirst, L)
};
static BwdSchedule bwd_schedule(const dsdgp_model* m) {
  const int L = m->desc.L;
  BwdSchedule s{}; s.overlap = overlap_on(m, m->fwd.n, m->fwd.S);
  const int g = s.gfirst = m->desc.white ? 0 : m->grad_first;     // reverse mode stops below this layer (dsdgp_model_set_grad_first_layer)
  // data-parallel buckets: every layer's reduction, products, assembly and hyper-parameter gradients right behind its weight-gradient
  // products, then the caller's collective on that layer's segment of the gradient, on the stream the segment was produced on — the
  // exchange of the upper layers runs under the lower layers' backward chains (dsdgp_model_set_bucket_callback)
  s.bucketed = m->bucket_fn != nullptr && m->tail_ok && g == 0 && !m->fuse_adam.on;
  s.pipelined = s.bucketed || (s.overlap && m->force.pipe_tail != 0 && !m->desc.white);
  // Ku^-1, S_d (and KS, U, UU for the assembly) come from the side stream.  In the overlapped schedule the chains wait for the event
  // behind the first of those launches only (prepare_async: ev_kinv); the join with the side stream at the end of backward_layers — which
  // the assembly launches follow — covers the rest.  The per-layer tails (buckets) read KS / U inside the loop: they take the full join.
  s.kinv_only = s.overlap && !s.pipelined && !m->desc.white && m->kinv_pending && m->side_pending;
  // (q_mu, q_sqrt)-only gradients (dsdgp_model_set_grad_q_only): the lowest layer of the pass needs d/dq_mu = sum_r a mbar^T and
  // d/dq_sqrt_d = 2 tril(P_d q_sqrt_d), P_d = sum_r vbar_d a a^T — the forward pass's A and the upstream adjoints, nothing the backward
  // chain produces (E, GW, dX feed Z, the kernel hyper-parameters and the layers below): no chain, and only the A jobs of its products
  s.q_only = m->grad_q_only && !m->desc.white;
  // Deep models (round 5): only the products of layer gfirst + 1 go to the side stream (they run under the lowest chain, the one launch
  // with too few row blocks to fill the chip); those of the layers above follow the lowest layer's products on the main stream — no
  // event record / wait pair per layer (6 + 12 us) and no products squeezed in beside a chain that saturates the MFMA pipe anyway.
  // 5-layer config 3: 7.60 -> 7.37 ms per step; the 3-layer configs (one deferred launch) are within +-1 %, so the rule starts at
  // four layers in the pass.  (DSDGP_FORCE wg_defer = 0 / 2: off / on at any depth.)
  s.defer_upper = s.overlap && !s.pipelined && (m->force.wg_defer == 2 || (m->force.wg_defer < 0 && L - g >= 4));
  // the lowest layer's products ran on the main stream: its split-K reduction goes ahead of the join, so that the side stream's
  // completion signal (a just-in-time cross-stream wait costs ~12 us of idle time) travels while the main stream works
  s.red_ahead = s.overlap && !s.pipelined && g == 0 && L > 1 && m->force.red_ahead != 0;
  for (int l = g; l < L; ++l) {
    const LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    BwdSchedule::Layer& y = s.layer[l];
    const bool last = (l == L - 1), produced = last ? m->fwd.adjoints_from_lik : l >= 1;
    const int64_t nblk = m->fwd.layer[l].ld / 16;
    y.chain = !(s.q_only && l == g);
    const bool prologue = !produced && !last && y.chain && m->force.adj_fuse != 0 && !m->fwd.layer[l].c_saved && !St.gemm && sm_adj_fusable(v.Mp, nblk, v.D_in, v.D_out);
    y.adj = produced ? ADJ_PRODUCER : (prologue ? ADJ_PROLOGUE : ADJ_PREP);
    y.d_split = bwd_d_split(m->force.bwd_split, v.Mp, St.bpart != nullptr, nblk, v.D_out);
    // the lowest layer of the reverse pass keeps its products on the main stream: nothing is left to run them under, and the
    // join then waits for side-stream work that finished long ago instead of for a just-in-time signal
    const bool on_main = s.overlap && l == g && L - g > 1;
    y.products = (!s.overlap || on_main) ? PROD_MAIN : ((s.defer_upper && l >= g + 2) ? PROD_DEFERRED : PROD_SIDE);
  }
  return s;
}

// argument block of layer l's backward chain
static LayerBwdArgs fill_bwd_args(const dsdgp_model* m, int l, const BwdSchedule& sc) {
  const LayerState& St = m->L[l];
  const LayerDev& v = St.dev;
  const auto& R = m->fwd.layer[l];
  const int64_t n = m->fwd.n;
  LayerBwdArgs b{};
  b.X = R.X; b.Rin = R.Rin; b.D_in = v.D_in; b.D_out = v.D_out; b.M = v.M; b.DP4 = v.DP4;
  b.Zp = v.Zp; b.Zs = v.Zs; b.hyp = v.hyp; b.Kinv = v.Kinv; b.Linv = v.Linv; b.LinvT = v.LinvT; b.Sd = v.Sd; b.qmu4 = v.qmu4;
  b.Asave = St.A; b.Csave = R.c_saved ? St.C : nullptr; b.Tp = v.Tp; b.TpT = v.TpT; b.ldA = R.ld; b.VB = St.VB; b.MB = St.MB;
  b.E = v.alg_g ? nullptr : St.E; b.GW = St.GW;
  b.dX = (l > sc.gfirst) ? m->L[l - 1].dF : nullptr;
  if (l >= 2 && l > sc.gfirst) {   // the previous layer is an inner layer: hand it its transposed adjoints directly
    const LayerState& Pv = m->L[l - 1];
    const auto& Rp = m->fwd.layer[l - 1];
    b.dX = nullptr;
    b.MBp = Pv.MB; b.VBp = Pv.VB;
    b.zp = Rp.z; b.zp_s = Rp.zs_s; b.zp_n = Rp.zs_n; b.zp_d = Rp.zs_d; b.n_inner = n;
    b.varp = Pv.var; b.Dp = Pv.dev.D_out; b.prop = Pv.prop; b.jitter = m->desc.jitter;
  }
  b.mean_kind = St.d.mean_kind; b.mean_A = St.meanA; b.hyp_part = St.hyp_part;
  if (sc.layer[l].adj == ADJ_PROLOGUE) {
    b.up_dF = St.dF; b.up_rep = R.rep; b.up_ld = v.D_out + St.prop; b.up_off = St.prop;
    b.up_z = R.z; b.up_zs = R.zs_s; b.up_zn = R.zs_n; b.up_zd = R.zs_d; b.up_n_inner = n;
    b.up_var = St.var; b.up_jitter = m->desc.jitter; b.MBw = St.MB; b.VBw = St.VB;
  }
  b.d_split = sc.layer[l].d_split; b.part = St.bpart; b.part_cnt = St.bcnt;
  return b;
}

// split-K reductions of the layers [first, end): their jobs and blocks are contiguous in the plan (ordered by layer)
static int launch_reduce(dsdgp_model* m, int first, int end, hipStream_t st) {
  const LayerState& S0 = m->L[first];
  const int njobs = (end < m->desc.L ? m->L[end].red_off : m->n_red) - S0.red_off;
  const int nblk = (end < m->desc.L ? m->L[end].red_blk0 : m->red_blocks) - S0.red_blk0;
  DS_LAUNCH(k_reduce_grouped, dim3(nblk), dim3(256), m->red_lds, st, m->rjobs + S0.red_off, njobs, S0.red_blk0);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}
// (a layer without a backward chain — q_only, the lowest — has only the A jobs of its products)
static int launch_wgrad(dsdgp_model* m, const BwdSchedule& sc, int l, hipStream_t st) {
  const LayerState& Sx = m->L[l];
  const bool all = sc.layer[l].chain;
  const int64_t ld = m->fwd.layer[l].ld;
  return wgrad_launch(m->ctx, Sx.wj, all ? Sx.njobs : Sx.njobsA, all ? Sx.tot_big : Sx.totA, Sx.ns_big, ld, ld, st);
}
// split-K reduction + P_d T_d / GS_d products of one layer right behind its weight-gradient products (pipelined tail); bucketed:
// its assembly and the caller's collective on its segment of the gradient as well
static int layer_tail(dsdgp_model* m, const BwdSchedule& sc, int l, hipStream_t st, double kl_weight) {
  const LayerState& St = m->L[l];
  DS_TRY(launch_reduce(m, l, l + 1, st));
  DS_TRY(gemm_launch(m->ctx, lq_pt(St), St.lq_np, St.lq_tp, st));
  if (sc.bucketed) {
    DS_LAUNCH(k_asm_rows, dim3(St.dev.M, 1), dim3(256), (size_t)m->mp_max_all * sizeof(double), st, (const LayerDev*)(m->layers_dev + l), m->grad,
              kl_weight, m->mp_max_all, m->force.asm_pre);
    DS_LAUNCH(k_tail, dim3(1), dim3(256), 0, st, m->layers_dev, l, 1, m->grad, FinArgs{}, AdamArgs{});
    DS_HIP(hipGetLastError());
    const int64_t lo = theta_segment_lo(m, l);
    m->bucket_fn(m->bucket_user, l, m->grad + lo, theta_segment_lo(m, l + 1) - lo, (void*)st);
  }
  return DSDGP_OK;
}

// The three endings of a reverse pass.  Bucketed: the last bucket — likelihood-variance gradient and the four result scalars (contiguous behind the layers' segments when
// `out` is grad + n_theta, as the contract of dsdgp_allreduce asks)
static int end_last_bucket(dsdgp_model* m, hipStream_t st) {
  const int L = m->desc.L;
  DS_LAUNCH(k_tail, dim3(1), dim3(256), 0, st, m->layers_dev, 0, 0, m->grad, fin_args(m), AdamArgs{});
  DS_HIP(hipGetLastError());
  m->fin.done = true;
  const int64_t lo = theta_segment_lo(m, L);
  const bool tail_scalars = m->fin.out == m->grad + m->desc.n_theta;
  m->bucket_fn(m->bucket_user, L, m->grad + lo, (m->desc.n_theta - lo) + (tail_scalars ? 4 : 0), (void*)st);
  if (!tail_scalars) m->bucket_fn(m->bucket_user, L + 1, m->fin.out, 4, (void*)st);
  return DSDGP_OK;
}
// tail_ok: one wave per inducing row (k_asm_rows), then hyper-parameter gradients, value and — in a training step — Adam (k_tail)
static int end_rows_tail(dsdgp_model* m, hipStream_t st, int gfirst, int La, double kl_weight) {
  DS_LAUNCH(k_asm_rows, dim3(m->m_max_all, La), dim3(256), (size_t)m->mp_max_all * sizeof(double), st, (const LayerDev*)(m->layers_dev + gfirst),
            m->grad, kl_weight, m->mp_max_all, m->force.asm_pre);
  AdamArgs A{m->theta, m->adam_m, m->adam_v, m->mask, m->desc.n_theta, m->fuse_adam.lr_t, m->fuse_adam.b1, m->fuse_adam.b2,
             m->fuse_adam.eps, (m->fuse_adam.on && gfirst == 0) ? 1 : 0};
  const int nadam = A.on ? (int)std::min<int64_t>(2048, ceil_div(m->desc.n_theta, 512)) : 0;      // a thread per pair of entries, eight workgroups per CU
  DS_LAUNCH(k_tail, dim3(La + 1 + nadam), dim3(256), 0, st, m->layers_dev, gfirst, La, m->grad, fin_args(m), A);
  DS_HIP(hipGetLastError());
  m->fin.done = true;
  return DSDGP_OK;
}
// white=True / wide inputs: the unfused assembly (the value follows in k_finalize)
static int end_unfused(dsdgp_model* m, hipStream_t st, const LayerDev* lay, int La, double kl_weight) {
  DS_LAUNCH(k_asm_kbar, dim3(m->kuu_blocks, La), dim3(256), 0, st, lay, kl_weight);
  if (m->n_wz) DS_TRY(gemm_launch(m->ctx, m->gp_wz, m->n_wz, m->t_wz));   // (wm of the layers below gfirst is stale: their WZ is never read)
  if (m->need_hyp_part) DS_LAUNCH(k_asm_hyp_part, dim3(NPART, La), dim3(256), 0, st, lay);
  DS_LAUNCH(k_asm_params, dim3(m->asm_blocks + 1, La), dim3(256), 0, st, lay, m->grad, kl_weight);
  DS_HIP(hipGetLastError());
  return DSDGP_OK;
}

// Reverse pass.  Streams (when the launches are long enough to pay for cross-stream events, overlap_on):
//   main : backward chain L-1, L-2, ..., gfirst, the weight-gradient products of layer gfirst, its split-K reduction | join | the
//          other layers' reduction, P_d T_d / GS_d products, gradient assembly, value + Adam
//   side : the weight-gradient products of layer l behind an event at the end of ITS backward chain, i.e. under the chain of layer
//          l - 1 (they fill the MFMA pipe while that chain's workgroups sit in their load / reduction phases and in the launch's
//          tail); with the pipelined tail (data-parallel buckets) also that layer's reduction, products and assembly.
// Every reduction is fixed-order, so the schedule does not change a bit of the result (tests/test_gpu_parity.py:
// test_stream_overlap_is_bitwise_neutral, tests/test_gpu_round3.py).
// The decisions are bwd_schedule's; here: wait, the layers (adjoint producer -> chain -> products), reductions, join, ending.
static int backward_layers(dsdgp_model* m, double kl_weight) {
  dsdgp_ctx* ctx = m->ctx;
  const int L = m->desc.L;
  const int64_t n = m->fwd.n;
  DS_TRY(ensure_plan(m, n, m->fwd.S));
  const BwdSchedule sc = bwd_schedule(m);
  const int gfirst = sc.gfirst;
  if (sc.kinv_only) DS_HIP(hipStreamWaitEvent(ctx->stream, m->ev_kinv, 0));
  else DS_TRY(join_prep(m));
  for (int l = L - 1; l >= gfirst; --l) {
    LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    const bool last = (l == L - 1);
    const auto& R = m->fwd.layer[l];
    const int64_t ld = R.ld;
    if (sc.layer[l].adj == ADJ_PREP)
      DS_LAUNCH(k_adj_prep, dim3(ceil_div(ld, 256), std::max(v.DP16, v.DinP16)), dim3(256), 0, ctx->stream, last ? nullptr : St.dF,
                         last ? m->lik_dmean : nullptr, last ? m->lik_dvar : nullptr, R.z, R.zs_s, R.zs_n,
                         R.zs_d, n, St.var, R.X, R.Rin, R.rep, v.D_in, v.D_out, v.DP16, v.DinP16, m->desc.jitter, ld,
                         St.MB, St.VB, St.XT1, v.D_out + St.prop, St.prop);
    DS_HIP(hipGetLastError());
    const LayerBwdArgs b = fill_bwd_args(m, l, sc);
    if (last && m->fwd.last_pending) {
      DS_TRY(layer_last_launch(ctx, m->fwd.last_fwd, b, v.Mp, v.kern_kind, m->fwd.hyp_rows));
      m->fwd.last_launched();
    } else if (!sc.layer[l].chain) { /* nothing downstream of this layer's chain is wanted */ }
    else if (St.gemm) DS_TRY(layer_bwd_gemm_launch(ctx, b, v.Mp, v.kern_kind, m->desc.white ? 1 : 0, m->gws));
    else DS_TRY(layer_bwd_sm_launch(ctx, b, v.Mp, v.kern_kind, m->desc.white));
    // in-launch split-K reduction: what is left for k_reduce_grouped of this layer are the chain's hyper-parameter partials — added
    // right behind the chain (a handful of workgroups beside the side stream's products) instead of in a launch behind the final join
    if (sc.layer[l].products == PROD_MAIN) {
      DS_TRY(launch_wgrad(m, sc, l, ctx->stream));
      for (int lu = l + 1; lu < L; ++lu)
        if (sc.layer[lu].products == PROD_DEFERRED) DS_TRY(launch_wgrad(m, sc, lu, ctx->stream));
      if (sc.pipelined) DS_TRY(layer_tail(m, sc, l, ctx->stream, kl_weight));
    } else if (sc.layer[l].products == PROD_SIDE) {
      // ONE event per chain boundary (an event record costs the recording stream ~6 us): behind it the side stream takes this layer's
      // products, which then run under the NEXT layer's backward chain.  Measured slower and removed in round 3: the products of a layer
      // ahead of its own chain's end (they need only the upstream adjoints), completion events attached to the chain / product launches
      // (hipExtLaunchKernelGGL: +3 us), a cap on the split count.
      DS_HIP(hipEventRecord(m->ev_bwd[l], ctx->stream));
      DS_HIP(hipStreamWaitEvent(m->side, m->ev_bwd[l], 0));
      DS_TRY(launch_wgrad(m, sc, l, m->side));
      if (sc.pipelined) DS_TRY(layer_tail(m, sc, l, m->side, kl_weight));
    }
  }
  if (sc.red_ahead) DS_TRY(launch_reduce(m, 0, 1, ctx->stream));
  if (sc.overlap) {
    // value + likelihood-variance gradient: needs the likelihood partials (main, before ev_bwd) and KL (side).  AFTER the
    // weight-gradient launches: its single workgroup was observed to sit for > 1 ms behind the co-running large-M chain, and
    // everything queued behind it on this stream waited with it
    if (!m->fin.done && !m->tail_ok) DS_TRY(launch_finalize(m, m->side));
    DS_HIP(hipEventRecord(m->ev_side, m->side));
    DS_HIP(hipStreamWaitEvent(ctx->stream, m->ev_side, 0));
    m->side_pending = false;      // (in order behind the parameter products: this join is theirs too)
  }
  if (!sc.pipelined) {
    // (the partial sums of the layers below a pruned pass are stale: their jobs — ordered by layer — are left out)
    DS_TRY(launch_reduce(m, sc.red_ahead ? 1 : gfirst, L, ctx->stream));
    if (m->desc.white) {
      DS_LAUNCH(k_white_lbar, dim3(32, L), dim3(256), 0, ctx->stream, m->layers_dev);
      DS_TRY(gemm_launch(ctx, m->gp_w1, 2 * L, m->t_w1));
      DS_LAUNCH(k_white_phi, dim3(32, L), dim3(256), 0, ctx->stream, m->layers_dev);
      DS_TRY(gemm_launch(ctx, m->gp_w2, L, m->t_w2));
      DS_TRY(gemm_launch(ctx, m->gp_w3, L, m->t_w3));
    } else if (gfirst > 0) {
      for (int l = gfirst; l < L; ++l) DS_TRY(gemm_launch(ctx, lq_pt(m->L[l]), m->L[l].lq_np, m->L[l].lq_tp));
    } else {
      DS_TRY(gemm_launch(ctx, m->gp_pt, m->n_pt, m->t_pt));
    }
  }
  // the assembly of the layers that took part (their gradient entries; those of the layers below gfirst keep their old content)
  if (sc.bucketed) return end_last_bucket(m, ctx->stream);
  if (m->tail_ok) return end_rows_tail(m, ctx->stream, gfirst, L - gfirst, kl_weight);
  return end_unfused(m, ctx->stream, m->layers_dev + gfirst, L - gfirst, kl_weight);
}

// the value (and the likelihood parameter's gradient) where the reverse pass's ending has not produced it: m->fin
static int finish_value(dsdgp_model* m) {
  if (!m->fin.done) {
    DS_TRY(join_prep(m));   // KL values
    DS_TRY(launch_finalize(m, m->ctx->stream));
  }
  return DSDGP_OK;
}

static int elbo_impl(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                     const int64_t* zstride, uint64_t seed, double data_scale, double kl_weight, int with_grad, double* out,
                     const GatherSrc* gs) {
  DS_CHECK_ARG(m && out && ((X && Y) || gs));
  DS_CHECK_ARG(!zs || zstride);
  DS_CHECK_ARG(!m->sample_w || S == m->sample_w_S);
  if (with_grad) {
    DS_CHECK_ARG(m->grad != nullptr);
  }
  dsdgp_ctx* ctx = m->ctx;
  if (gs) {      // (gathered by forward_pass, on its way to prepare)
    X = m->Xmb;
    Y = m->Ymb;
  }
  const double w = data_scale / (double)S;
  const FwdCall c{X, n, S, zs, zstride, seed, nullptr, nullptr, nullptr, Y, w};
  FwdPlan p;
  DS_TRY(forward_pass(m, c, fwd_in(m, c, true, with_grad != 0, false, true), gs, &p));
  LayerState& last = m->L[m->desc.L - 1];
  const int DY = last.dev.D_out;
  const bool own_adj = with_grad && !p.adjoints_from_lik;      // the adjoints go to lik_dmean / lik_dvar: k_adj_prep transposes them
  if (p.lik == LIK_ELEMENTWISE) {
    const int64_t ldt = round_up((int64_t)S * n, 16);
    double* mbt = p.adjoints_from_lik ? last.MB : nullptr;
    double* vbt = p.adjoints_from_lik ? last.VB : nullptr;
    lik_dispatch(m->desc.lik_kind, [&](auto fam) {
      DS_LAUNCH(k_lik_elbo<decltype(fam)::value>, dim3(p.lik_nblocks), dim3(256), 0, ctx->stream, (int)m->desc.lik_kind, (const double*)m->lik_const,
                m->desc.lik_aux, last.mean, last.var, Y, n, S, DY, w, m->sample_w, m->lik_part, own_adj ? m->lik_dmean : nullptr,
                own_adj ? m->lik_dvar : nullptr, mbt, vbt, ldt);
    });
  } else if (p.lik == LIK_MULTICLASS) {
    // MultiClass: Y is (n x 1) labels, the last layer has K = num_classes outputs; ve per (s, i) row -> last.F scratch
    DS_CHECK_ARG(DY == m->desc.num_classes);
    const int64_t R = (int64_t)S * n;
    DS_TRY(multiclass_launch(ctx, last.mean, last.var, Y, n, R, DY, 0, w, last.F, with_grad ? m->lik_dmean : nullptr,
                             with_grad ? m->lik_dvar : nullptr, -1));
    if (m->sample_w) {
      const int64_t cnt = R * DY;
      DS_LAUNCH(k_scale_by_sample, dim3((int)std::min<int64_t>(2048, ceil_div(cnt, 256))), dim3(256), 0, ctx->stream,
                         m->sample_w, n, S, DY, R, last.F, with_grad ? m->lik_dmean : nullptr, with_grad ? m->lik_dvar : nullptr);
    }
    DS_LAUNCH(k_partial_sum, dim3(p.lik_nblocks), dim3(256), 0, ctx->stream, last.F, R, m->lik_part);
  }
  DS_HIP(hipGetLastError());
  m->fin.nblocks = p.lik_nblocks; m->fin.w = w; m->fin.kl_weight = kl_weight; m->fin.with_grad = with_grad; m->fin.out = out;
  m->fin.done = false;
  if (with_grad) {
    DS_TRY(backward_layers(m, kl_weight));
    m->ps.grad_evaluated(pass_is_pruned(m->desc.white, m->grad_first, m->grad_q_only));
  }
  return finish_value(m);
}

extern "C" int dsdgp_model_elbo(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S,
                                const double* const* zs, const int64_t* zstride, uint64_t seed, double data_scale,
                                double kl_weight, int with_grad, double* out) {
  DS_CHECK_ARG(X && Y);
  return elbo_impl(m, X, Y, n, S, zs, zstride, seed, data_scale, kl_weight, with_grad, out, nullptr);
}

// Vector-Jacobian product of the layers (model_zoo.py:52-57: the collapsed bound differentiated through the inner layers).  The forward
// half: the front of elbo_impl(with_grad = 1) — draws, prepare with the gradient-side products, chains with save — and no likelihood
// (lik_Y null: neither the fused last launch of layer_last.hip nor the likelihood-in-epilogue instance is taken), no sample of the last layer.
static int vjp_refusals(const char* who, const dsdgp_model* m) {
  if (m->bucket_fn) {
    dsdgp_set_error("%s: a bucket callback is set (dsdgp_model_set_bucket_callback); the vector-Jacobian product is single-process", who);
    return DSDGP_ERR_UNSUPPORTED;
  }
  if (m->sample_w) {
    dsdgp_set_error("%s: quadrature sample weights are set (dsdgp_model_set_sample_weights); the caller's adjoints carry their own weights", who);
    return DSDGP_ERR_UNSUPPORTED;
  }
  if (pass_is_pruned(m->desc.white, m->grad_first, m->grad_q_only)) {
    dsdgp_set_error("%s: the reverse pass is restricted to layers >= %d%s (dsdgp_model_set_grad_first_layer / _q_only)", who, m->grad_first,
                    m->grad_q_only ? ", (q_mu, q_sqrt) only" : "");
    return DSDGP_ERR_BAD_ARG;
  }
  return DSDGP_OK;
}
extern "C" int dsdgp_model_forward_saved(dsdgp_model* m, const double* X, int64_t n, int32_t S, const double* const* zs,
                                         const int64_t* zstride, uint64_t seed, double* mean_out, double* var_out) {
  DS_CHECK_ARG(m && X && m->grad != nullptr);
  DS_CHECK_ARG(!zs || zstride);
  DS_CHECK_ARG(n > 0 && n <= m->n_max && S > 0 && S <= m->s_max);
  DS_TRY(vjp_refusals("dsdgp_model_forward_saved", m));
  dsdgp_ctx* ctx = m->ctx;
  const FwdCall c{X, n, S, zs, zstride, seed, nullptr, nullptr, nullptr, nullptr, 0.0};
  DS_TRY(forward_pass(m, c, fwd_in(m, c, true, true, false, false)));
  const LayerState& last = m->L[m->desc.L - 1];
  const size_t bytes = (size_t)S * n * last.dev.D_out * sizeof(double);
  if (mean_out) DS_HIP(hipMemcpyAsync(mean_out, last.mean, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (var_out) DS_HIP(hipMemcpyAsync(var_out, last.var, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  m->ps.saved_recorded(n, S);
  return DSDGP_OK;
}
// The reverse half: the last layer's adjoints are the caller's (ADJ_PREP reads them from lik_dmean / lik_dvar, as after MultiClass), no
// likelihood block takes part in the value (fin.nblocks = 0: lik_part is not read).
extern "C" int dsdgp_model_backward_adjoints(dsdgp_model* m, const double* dmean, const double* dvar, double kl_weight, double* out) {
  DS_CHECK_ARG(m && dmean && dvar && out && m->grad != nullptr);
  if (!m->ps.saved) {
    dsdgp_set_error("dsdgp_model_backward_adjoints: the model's last evaluation is not a dsdgp_model_forward_saved (another evaluation, a "
                    "change of theta or an optimiser step since then drops the saved forward pass)");
    return DSDGP_ERR_BAD_ARG;
  }
  DS_TRY(vjp_refusals("dsdgp_model_backward_adjoints", m));
  dsdgp_ctx* ctx = m->ctx;
  const int64_t n = m->ps.saved_n;
  const int S = m->ps.saved_S;
  m->ps.saved_consumed();
  const int64_t count = (int64_t)S * n * m->L[m->desc.L - 1].dev.D_out;      // <= s_max n_max D_out, the size of lik_dmean / lik_dvar
  DS_LAUNCH(k_seed_adjoints, dim3((int)std::min<int64_t>(2048, ceil_div(count, 256))), dim3(256), 0, ctx->stream, dmean, dvar, count,
            m->lik_dmean, m->lik_dvar);
  DS_HIP(hipGetLastError());
  m->fwd.adjoints_from_caller();
  m->fin.nblocks = 0; m->fin.w = 0.0; m->fin.kl_weight = kl_weight; m->fin.with_grad = 1; m->fin.out = out;
  m->fin.done = false;
  DS_TRY(backward_layers(m, kl_weight));
  m->ps.grad_evaluated(false);
  DS_TRY(finish_value(m));
  // every ending writes -w * (sum of no partials) * sigmoid(raw) = -0.0 there: the entry is +0.0
  const int64_t ol = lik_var_offset(m);
  if (ol >= 0) DS_HIP(hipMemsetAsync(m->grad + ol, 0, sizeof(double), ctx->stream));
  return DSDGP_OK;
}

extern "C" int dsdgp_model_set_sample_weights(dsdgp_model* m, const double* w, int32_t S) {
  DS_CHECK_ARG(m && (!w || (S > 0 && S <= m->s_max)));
  m->sample_w = w;
  m->sample_w_S = w ? S : 0;
  return DSDGP_OK;
}

// Adam's bias-corrected step size at step t
static double adam_lr_t(double lr, double b1, double b2, int64_t t) { return lr * sqrt(1.0 - pow(b2, (double)t)) / (1.0 - pow(b1, (double)t)); }

extern "C" int dsdgp_model_adam_step(dsdgp_model* m, double lr, double beta1, double beta2, double eps, int64_t t) {
  DS_CHECK_ARG(m && m->grad && m->adam_m && m->adam_v && t >= 1);
  if (m->ps.grad_pruned) {
    dsdgp_set_error("dsdgp_model_adam_step: the last gradient was evaluated for layers >= %d only (dsdgp_model_set_grad_first_layer)", m->grad_first);
    return DSDGP_ERR_BAD_ARG;
  }
  const double lr_t = adam_lr_t(lr, beta1, beta2, t);
  const int64_t n = m->desc.n_theta;
  const int nb = (int)std::min<int64_t>(2048, ceil_div(n, 512));      // a thread per pair of entries (adam_sweep), eight workgroups per CU
  DS_LAUNCH(k_adam, dim3(nb), dim3(256), 0, m->ctx->stream, m->theta, m->grad, m->adam_m, m->adam_v, m->mask, n,
                     lr_t, beta1, beta2, eps, (const LayerDev*)m->layers_dev, m->desc.L);
  DS_HIP(hipGetLastError());
  m->ps.theta_moved();
  return DSDGP_OK;
}

// One optimiser step in one call: ELBO + gradient with the Adam update applied by the tail launch of the reverse pass (no separate
// k_adam launch; `session.run(opt_op)` of demos/demo_regression_UCI.ipynb:324).  Falls back to elbo + adam_step where the fused tail
// does not apply (white=True, wide inputs).
static int train_step_impl(dsdgp_model* m, const double* X, const double* Y, int64_t n, int32_t S, const double* const* zs,
                           const int64_t* zstride, uint64_t seed, double data_scale, double kl_weight, double lr, double beta1,
                           double beta2, double eps, int64_t t, double* out, const GatherSrc* gs) {
  DS_CHECK_ARG(m && m->grad && m->adam_m && m->adam_v && t >= 1);
  if (pass_is_pruned(m->desc.white, m->grad_first, m->grad_q_only)) {
    dsdgp_set_error("dsdgp_model_train_step: the reverse pass is restricted to layers >= %d%s (dsdgp_model_set_grad_first_layer / _q_only)",
                    m->grad_first, m->grad_q_only ? ", (q_mu, q_sqrt) only" : "");
    return DSDGP_ERR_BAD_ARG;
  }
  if (!m->tail_ok) {
    DS_TRY(elbo_impl(m, X, Y, n, S, zs, zstride, seed, data_scale, kl_weight, 1, out, gs));
    return dsdgp_model_adam_step(m, lr, beta1, beta2, eps, t);
  }
  m->fuse_adam.on = 1;
  m->fuse_adam.lr_t = adam_lr_t(lr, beta1, beta2, t);
  m->fuse_adam.b1 = beta1; m->fuse_adam.b2 = beta2; m->fuse_adam.eps = eps;
  const int rc = elbo_impl(m, X, Y, n, S, zs, zstride, seed, data_scale, kl_weight, 1, out, gs);
  m->fuse_adam.on = 0;
  DS_TRY(rc);
  m->ps.theta_moved();
  return DSDGP_OK;
}
