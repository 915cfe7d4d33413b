// Stand-alone check of the forward plan (csrc/forward_plan.hpp, csrc/chain_policy.hpp) on the CPU.
//   (a) legacy::decide is a transcription of the conditions the forward pass took inline before the plan existed (forward_layers,
//       last_chain_fusable, layer_last_fusable, bwd_d_split, inner_draws, the block counts of elbo_impl): fwd_plan must agree with it,
//       field by field, over a grid that straddles every threshold of the rules;
//   (b) invariants of the plan that do not depend on the transcription;
//   (c) a table that pins the plans of the benchmark configurations and of config 2's per-GPU shards.
// Exit 1 with a message on the first violation.  Built and run by tests/test_forward_plan_cpu.py (system C++ compiler, address +
// undefined sanitizers).
#include "chain_policy.hpp"
#include "forward_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string>

static const FwdIn* g_in;
static std::string g_case;
static std::string describe() {
  const FwdIn& in = *g_in;
  char t[512];
  snprintf(t, sizeof t, "%s n %lld S %d prepare %d save %d need_last_F %d lik_target %d sample_w %d with_grad %d caller_z %x | L %d white %d elementwise %d "
           "gaussian %d grad_first %d q_only %d head_ok %d overlap %d timing %d | force white_fwd %d cs %d %d %d last_fuse %d last_min_blocks %d bwd_split %d "
           "lik_fuse %d\n", g_case.c_str(), (long long)in.n, in.S, in.prepare, in.save, in.need_last_F, in.lik_target, in.sample_w, in.with_grad, in.caller_z,
           in.L, in.white, in.lik_elementwise, in.lik_gaussian, in.grad_first, in.grad_q_only, in.head_ok, in.overlap, in.timing, in.force.white_fwd,
           in.force.cs_min_blocks, in.force.cs_min_dout, in.force.cs_max_dout, in.force.last_fuse, in.force.last_min_blocks, in.force.bwd_split,
           in.force.lik_fuse);
  std::string s = t;
  for (int l = 0; l < in.L; ++l) {
    const FwdIn::Layer& v = in.layer[l];
    snprintf(t, sizeof t, "  layer %d: Mp %d D_in %d D_out %d kern %d mean %d prop %d gemm %d alg_g %d need_tpt %d has_C %d has_bpart %d\n", l, v.Mp, v.D_in,
             v.D_out, v.kern_kind, v.mean_kind, v.prop, v.gemm, v.alg_g, v.need_tpt, v.has_C, v.has_bpart);
    s += t;
  }
  return s;
}
#define REQUIRE(cond, ...)                                                                 \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      fprintf(stderr, "forward_check: %s  violated: %s\n  ", describe().c_str(), #cond);  \
      fprintf(stderr, __VA_ARGS__);                                                        \
      fprintf(stderr, "\n");                                                               \
      exit(1);                                                                             \
    }                                                                                      \
  } while (0)

// ---- (a) the decisions as the forward pass took them inline.  The model and the argument block carry what those conditions read, under
// the names they read it by; pointers are booleans (set or null).  The size rules they call (sm_hyp_parts, sm_cs_built, chain_d_split,
// layer_last_built, layer_gemm_lik_blocks) moved to chain_policy.hpp unchanged and are called here as they were there.
namespace legacy {
struct LayerDev { int Mp, D_in, D_out, kern_kind, alg_g, need_tpt; };
struct LayerState { LayerDev dev; struct { int mean_kind; } d; bool C, bpart, gemm; int prop; };
struct Model {
  struct { int L; bool white; int lik_kind; } desc;
  int grad_first; bool grad_q_only, head_ok, sample_w, timing;
  LayerState L[DSDGP_MAX_LAYERS];
  struct { int cs_min_blocks, cs_min_dout, cs_max_dout, bwd_split, lik_fuse, white_fwd, last_fuse, last_min_blocks; } force;
};
struct LayerFwdArgs { int64_t Rin, ldA; int rep, D_in, D_out, qmu_ld, mean_kind, d_split; bool z, z_caller, F, Asave, Csave, XT1, lik_Y; };
struct Out {
  bool join_prep, z_head, z_side, fork_side, fused_last, lik_in_chain;
  int hr_nblk, nblocks;
  struct Layer { LayerFwdArgs a; bool wf, want_F, drawn_here, deferred, gemm_launch, concat; } layer[DSDGP_MAX_LAYERS];
  int hyp_rows, bwd_split_last;
};

static bool elementwise(int kind) { return kind != DSDGP_LIK_MULTICLASS; }      // lik_family(kind) != LIKF_NONE for the kinds a model can have
static int bwd_d_split(const Model* m, const LayerState& St, int64_t nblk) {
  const bool want = m->force.bwd_split >= 2 || (m->force.bwd_split == 1 && St.dev.Mp > 256);
  return (want && St.bpart) ? chain_d_split(nblk, St.dev.D_out) : 1;
}
static int layer_last_fusable(const LayerFwdArgs& a, int Mp, int kern_kind, int hyp_rows, int bwd_d_split, int want_E) {
  const int waves = Mp == 128 ? 4 : 8;
  return layer_last_built(Mp, a.D_in, a.D_out) && (kern_kind == DSDGP_KERN_RBF || kern_kind == DSDGP_KERN_MATERN52) && hyp_rows >= waves &&
         a.lik_Y && a.Asave && !a.Csave && !a.F && a.rep == 1 && !a.qmu_ld && a.mean_kind == DSDGP_MEAN_ZERO && a.d_split <= 1 &&
         bwd_d_split <= 1 && !want_E;
}
static bool last_chain_fusable(const Model* m, const LayerState& St, const LayerFwdArgs& a) {
  const LayerDev& v = St.dev;
  if (m->force.last_fuse == 0 || m->force.bwd_split >= 2 || !v.need_tpt || m->desc.white || St.gemm || m->desc.L < 2) return false;
  if (m->grad_q_only && m->grad_first == m->desc.L - 1) return false;
  if (m->timing || ceil_div(a.Rin, 16) < m->force.last_min_blocks) return false;
  const int hyp_rows = (int)(sm_hyp_parts(a.ldA, v.Mp, v.D_in) / (a.ldA / 16));
  return layer_last_fusable(a, v.Mp, v.kern_kind, hyp_rows, bwd_d_split(m, St, a.ldA / 16), !v.alg_g);
}
static void forward_layers(const Model* m, int64_t n, int S, uint32_t zs, bool save, bool need_last_F, bool z_ready, bool lik_Y, int* lik_nblocks, Out& o) {
  const int L = m->desc.L;
  const bool wf_ok = !m->desc.white && !save && m->force.white_fwd != 0;
  o.join_prep = wf_ok;
  for (int l = 0; l < L; ++l) {
    const LayerState& St = m->L[l];
    const LayerDev& v = St.dev;
    const int64_t Rin = (l == 0) ? n : (int64_t)S * n;
    const int rep = (l == 0) ? S : 1;
    const bool last = (l == L - 1);
    const bool want_F = !last || need_last_F;
    const bool wf = wf_ok && v.Mp <= 256 && !St.gemm;
    LayerFwdArgs a{};
    a.Rin = Rin; a.rep = rep;
    a.D_in = v.D_in; a.D_out = v.D_out;
    if (wf) a.qmu_ld = 4;
    a.mean_kind = St.d.mean_kind;
    bool drawn_here = false;
    if (want_F) {
      if (zs >> l & 1) {
        a.z = a.z_caller = true;
      } else {
        if (!(z_ready && !last)) drawn_here = true;
        a.z = true;
      }
    }
    a.F = want_F;
    a.ldA = round_up(Rin, 16);
    const bool save_l = save && (m->desc.white || l >= m->grad_first);
    a.Asave = save_l;
    bool c_used = save_l && St.C && sm_cs_built(v.Mp) &&
                  (v.Mp > 256 || ((Rin + 15) / 16 > m->force.cs_min_blocks && v.D_out >= m->force.cs_min_dout && v.D_out <= m->force.cs_max_dout));
    if (St.gemm) c_used = save_l && St.C;
    const bool q_lowest = save_l && m->grad_q_only && !m->desc.white && l == m->grad_first;
    if (q_lowest) c_used = false;
    a.Csave = c_used;
    a.XT1 = save_l && !q_lowest;
    {
      const int64_t nblk = (Rin + 15) / 16;
      a.d_split = chain_d_split(nblk, v.D_out);
      if (last && lik_Y) {
        a.lik_Y = true;
        *lik_nblocks = St.gemm ? layer_gemm_lik_blocks(Rin, v.D_out) : (int)nblk * a.d_split;
      }
    }
    Out::Layer& y = o.layer[l];
    y.deferred = last && last_chain_fusable(m, St, a);
    y.gemm_launch = !y.deferred && St.gemm;
    y.a = a; y.wf = wf; y.want_F = want_F; y.drawn_here = drawn_here;
    y.concat = St.prop && !last;
  }
  // what backward_layers recomputed at launch time from the recorded leading dimension
  const LayerState& St = m->L[L - 1];
  const int64_t ld = o.layer[L - 1].a.ldA;
  o.hyp_rows = (int)(sm_hyp_parts(ld, St.dev.Mp, St.dev.D_in) / (ld / 16));
  o.bwd_split_last = bwd_d_split(m, St, ld / 16);
}
static void inner_draws(const Model* m, int64_t n, int S, uint32_t zs, bool ovl, Out& o) {
  const int L = m->desc.L;
  if (m->head_ok) {
    for (int l = 0; l + 1 < L; ++l)
      if (!(zs >> l & 1)) {
        const int64_t count = (int64_t)S * n * m->L[l].dev.D_out;
        o.hr_nblk = std::max<int>(o.hr_nblk, (int)std::min<int64_t>(64, ceil_div((count + 1) / 2, 4 * 512)));
        o.z_head = true;
      }
  } else if (ovl) {
    o.fork_side = true;
    for (int l = 0; l + 1 < L; ++l)
      if (!(zs >> l & 1)) o.z_side = true;
  }
}
// prepare: elbo_impl / dsdgp_model_forward_saved (draws ahead, then the chains); else dsdgp_model_propagate / mixture_forward.
// lik_target: elbo_impl's likelihood part
static Out decide(const Model* m, int64_t n, int S, uint32_t zs, bool prepare, bool save, bool need_last_F, bool lik_target, bool with_grad, bool ovl) {
  Out o{};
  const int L = m->desc.L;
  if (prepare) inner_draws(m, n, S, zs, ovl, o);
  if (!lik_target) {
    int unused = 0;
    forward_layers(m, n, S, zs, save, need_last_F, o.z_side || o.z_head, false, &unused, o);
    return o;
  }
  const LayerState& last = m->L[L - 1];
  const int DY = last.dev.D_out;
  const int64_t total = (int64_t)S * n * DY;
  int nblocks = ceil_div(total, 256);
  o.fused_last = with_grad && L > 1 && elementwise(m->desc.lik_kind);
  o.lik_in_chain = o.fused_last && m->desc.lik_kind == DSDGP_LIK_GAUSSIAN && !m->sample_w && m->force.lik_fuse != 0;
  int lik_nb = 0;
  forward_layers(m, n, S, zs, save, need_last_F, o.z_side || o.z_head, o.lik_in_chain, &lik_nb, o);
  if (o.lik_in_chain) {
    nblocks = lik_nb;
  } else if (elementwise(m->desc.lik_kind)) {
    const int64_t ldt = round_up((int64_t)S * n, 16);
    if (o.fused_last) nblocks = ceil_div(ldt * DY, 256);
  } else {
    const int64_t R = (int64_t)S * n;
    nblocks = ceil_div(R, 256);
  }
  o.nblocks = nblocks;
  return o;
}
static Model model_of(const FwdIn& in) {
  Model m{};
  m.desc.L = in.L; m.desc.white = in.white;
  m.desc.lik_kind = in.lik_gaussian ? DSDGP_LIK_GAUSSIAN : (in.lik_elementwise ? DSDGP_LIK_BERNOULLI : DSDGP_LIK_MULTICLASS);
  m.grad_first = in.grad_first; m.grad_q_only = in.grad_q_only; m.head_ok = in.head_ok; m.sample_w = in.sample_w; m.timing = in.timing;
  for (int l = 0; l < in.L; ++l) {
    const FwdIn::Layer& v = in.layer[l];
    m.L[l] = LayerState{LayerDev{v.Mp, v.D_in, v.D_out, v.kern_kind, v.alg_g, v.need_tpt}, {v.mean_kind}, v.has_C, v.has_bpart, v.gemm, v.prop};
  }
  m.force = {in.force.cs_min_blocks, in.force.cs_min_dout, in.force.cs_max_dout, in.force.bwd_split, in.force.lik_fuse, in.force.white_fwd,
             in.force.last_fuse, in.force.last_min_blocks};
  return m;
}
}      // namespace legacy

static void check_against_legacy(const FwdIn& in, const FwdPlan& p) {
  const legacy::Model m = legacy::model_of(in);
  const legacy::Out o = legacy::decide(&m, in.n, in.S, in.caller_z, in.prepare, in.save, in.need_last_F, in.lik_target, in.with_grad, in.overlap);
  REQUIRE(p.join_prep_first == o.join_prep, "join_prep_first %d", p.join_prep_first);
  REQUIRE((p.draws == DRAWS_HEAD) == (in.prepare && in.head_ok) && (p.draws == DRAWS_SIDE) == o.fork_side, "draws %d, side fork %d", p.draws, o.fork_side);
  REQUIRE((p.draws == DRAWS_HEAD && p.draws_ahead) == o.z_head && (p.draws == DRAWS_SIDE && p.draws_ahead) == o.z_side && p.draws_ahead == (o.z_head || o.z_side),
          "draws %d ahead %d, z_head %d z_side %d", p.draws, p.draws_ahead, o.z_head, o.z_side);
  REQUIRE(p.head_nblk == o.hr_nblk, "head_nblk %d, hr.nblk %d", p.head_nblk, o.hr_nblk);
  REQUIRE(p.adjoints_from_lik == o.fused_last && p.lik_in_chain == o.lik_in_chain, "adjoints_from_lik %d lik_in_chain %d", p.adjoints_from_lik, p.lik_in_chain);
  const LikRoute route = !in.lik_target ? LIK_NONE : (o.lik_in_chain ? LIK_IN_CHAIN : (in.lik_elementwise ? LIK_ELEMENTWISE : LIK_MULTICLASS));
  REQUIRE(p.lik == route && p.lik_nblocks == o.nblocks, "likelihood route %d, blocks %d, nblocks %d", p.lik, p.lik_nblocks, o.nblocks);
  for (int l = 0; l < in.L; ++l) {
    const FwdPlan::Layer& y = p.layer[l];
    const legacy::Out::Layer& w = o.layer[l];
    REQUIRE(y.Rin == w.a.Rin && y.rep == w.a.rep && y.ld == w.a.ldA, "layer %d: Rin %lld rep %d ld %lld", l, (long long)y.Rin, y.rep, (long long)y.ld);
    REQUIRE(y.whitened == w.wf && y.whitened == (w.a.qmu_ld != 0) && y.want_F == w.want_F && y.want_F == w.a.F, "layer %d: whitened %d want_F %d", l, y.whitened, y.want_F);
    const DrawFrom draw = !w.a.z ? DRAW_NONE : (w.a.z_caller ? DRAW_CALLER : (w.drawn_here ? DRAW_HERE : DRAW_READY));
    REQUIRE(y.draw == draw, "layer %d: draw %d, was %d", l, y.draw, draw);
    REQUIRE(y.save_A == w.a.Asave && y.save_C == w.a.Csave && y.save_XT1 == w.a.XT1, "layer %d: save A %d C %d XT1 %d", l, y.save_A, y.save_C, y.save_XT1);
    REQUIRE(y.d_split == w.a.d_split && y.lik_epilogue == w.a.lik_Y, "layer %d: d_split %d lik_epilogue %d", l, y.d_split, y.lik_epilogue);
    const FwdLaunch launch = w.deferred ? LAUNCH_WITH_REVERSE : (w.gemm_launch ? LAUNCH_GEMM : LAUNCH_CHAIN);
    REQUIRE(y.launch == launch && y.concat == w.concat, "layer %d: launch %d, was %d; concat %d", l, y.launch, launch, y.concat);
  }
  REQUIRE(p.hyp_rows == o.hyp_rows && p.bwd_d_split == o.bwd_split_last, "hyp_rows %d (%d), backward d_split %d (%d)", p.hyp_rows, o.hyp_rows, p.bwd_d_split,
          o.bwd_split_last);
}

// ---- (b) what holds of every plan, whatever the rules say in detail
static void check_invariants(const FwdIn& in, const FwdPlan& p) {
  for (int l = 0; l < in.L; ++l) {
    const FwdIn::Layer& v = in.layer[l];
    const FwdPlan::Layer& y = p.layer[l];
    const bool last = l == in.L - 1;
    REQUIRE(!y.save_C || y.save_A, "layer %d keeps c_d without A", l);
    REQUIRE(!y.save_XT1 || y.save_A, "layer %d keeps [X^T;1] without A", l);
    REQUIRE(!y.save_A || in.save, "layer %d keeps A in a pass that saves nothing", l);
    if (!in.white && l < in.grad_first) REQUIRE(!y.save_A && !y.save_C && !y.save_XT1, "layer %d lies below the pruned reverse pass and keeps something", l);
    if (in.save && !in.white && in.grad_q_only && l == in.grad_first)
      REQUIRE(y.save_A && !y.save_C && !y.save_XT1, "the lowest layer (%d) of a (q_mu, q_sqrt)-only pass keeps A %d C %d XT1 %d", l, y.save_A, y.save_C, y.save_XT1);
    if (y.whitened) REQUIRE(!in.save && !in.white && v.Mp <= 256 && !v.gemm && y.launch == LAUNCH_CHAIN && p.join_prep_first, "layer %d whitened", l);
    if (y.launch == LAUNCH_WITH_REVERSE)
      REQUIRE(last && in.save && y.save_A && y.lik_epilogue && !y.want_F && !y.save_C && y.d_split == 1 && p.bwd_d_split == 1 && p.hyp_rows >= 4, "layer %d WITH_REVERSE", l);
    REQUIRE((y.launch == LAUNCH_GEMM) == v.gemm, "layer %d: launch %d, gemm %d", l, y.launch, v.gemm);
    if (y.lik_epilogue) REQUIRE(last && p.adjoints_from_lik && p.lik_in_chain && p.lik == LIK_IN_CHAIN && in.lik_target, "layer %d: likelihood epilogue", l);
    REQUIRE(y.want_F == (y.draw != DRAW_NONE), "layer %d: want_F %d, draw %d", l, y.want_F, y.draw);
    REQUIRE((y.draw == DRAW_CALLER) == (y.want_F && (in.caller_z >> l & 1)), "layer %d: draw %d, caller_z %x", l, y.draw, in.caller_z);
    if (!last) REQUIRE((y.draw == DRAW_READY) == (p.draws != DRAWS_INLINE && !(in.caller_z >> l & 1)), "inner layer %d: draw %d, placement %d", l, y.draw, p.draws);
    else REQUIRE(y.draw != DRAW_READY, "the last layer's draws are never made ahead");
    REQUIRE(y.d_split >= 1 && y.d_split <= 4 && y.d_split <= std::max(1, v.D_out), "layer %d: d_split %d", l, y.d_split);
    REQUIRE(y.ld % 16 == 0 && y.ld >= y.Rin && y.ld < y.Rin + 16, "layer %d: ld %lld", l, (long long)y.ld);
  }
  REQUIRE(p.draws == DRAWS_INLINE || in.prepare, "draws placed ahead of a prepare that the call does not run");
  REQUIRE(p.draws_ahead ? p.draws != DRAWS_INLINE : p.head_nblk == 0, "draws_ahead %d, placement %d, head blocks %d", p.draws_ahead, p.draws, p.head_nblk);
  REQUIRE((p.head_nblk > 0) == (p.draws == DRAWS_HEAD && p.draws_ahead) && p.head_nblk <= 64, "head blocks %d", p.head_nblk);
  REQUIRE(!p.lik_in_chain || p.adjoints_from_lik, "likelihood in the chain without its adjoints");
  REQUIRE(!p.adjoints_from_lik || (in.lik_target && in.with_grad && in.L > 1 && in.lik_elementwise), "adjoints_from_lik");
  REQUIRE((p.lik == LIK_NONE) == !in.lik_target && (p.lik == LIK_NONE ? p.lik_nblocks == 0 : p.lik_nblocks >= 1), "likelihood route %d, %d blocks", p.lik, p.lik_nblocks);
}

// the transitions of the record: what a reverse pass would read
struct Args { int tag; };
static void check_record(const FwdIn& in, const FwdPlan& p, FwdRecord<Args>& rec) {
  FwdUsed used[DSDGP_MAX_LAYERS];
  static const double X[DSDGP_MAX_LAYERS] = {0}, z[DSDGP_MAX_LAYERS] = {0};
  for (int l = 0; l < in.L; ++l) used[l] = FwdUsed{X + l, p.layer[l].draw == DRAW_NONE ? nullptr : z + l, 3 + l, 2, 1};
  const bool with_reverse = p.layer[in.L - 1].launch == LAUNCH_WITH_REVERSE;
  const Args a{(int)in.n};
  rec.forward_done(in, p, used, with_reverse ? &a : nullptr);
  REQUIRE(rec.n == in.n && rec.S == in.S && rec.adjoints_from_lik == p.adjoints_from_lik && rec.last_pending == with_reverse, "the record after a forward pass");
  REQUIRE(!with_reverse || (rec.last_fwd.tag == a.tag && rec.hyp_rows == p.hyp_rows), "the pending launch");
  for (int l = 0; l < in.L; ++l) {
    const auto& r = rec.layer[l];
    REQUIRE(r.X == X + l && r.z == used[l].z && r.zs_s == 3 + l && r.Rin == p.layer[l].Rin && r.ld == p.layer[l].ld && r.rep == p.layer[l].rep &&
            r.c_saved == p.layer[l].save_C, "layer %d of the record", l);
  }
  if (with_reverse) {
    rec.last_launched();
    REQUIRE(!rec.last_pending, "last_launched");
  }
}

// ---- the grid
static const int MPS[] = {32, 112, 128, 192, 256, 320, 512, 1024}, DINS[] = {1, 8, 16, 17, 64, 65}, DOUTS[] = {1, 2, 3, 5, 8, 30};
static const int BLOCKS[] = {159, 160, 161, 255, 256, 257, 511, 512, 513, 768, 769};      // row-block counts to straddle
struct Force { int white_fwd, save_c, cs_min_blocks, cs_min_dout, cs_max_dout, last_fuse, last_min_blocks, bwd_split, lik_fuse; };
static const Force FORCE_DEFAULT = {1, 1, 160, 3, 1 << 20, 1, 1, 1, 1};
// every forward-side field at its non-default values, one at a time, and the combination the parity tests use
static const Force FORCES[] = {FORCE_DEFAULT, {0, 1, 160, 3, 1 << 20, 1, 1, 1, 1}, {1, 0, 160, 3, 1 << 20, 1, 1, 1, 1}, {1, 2, 160, 3, 1 << 20, 1, 1, 1, 1},
                               {1, 2, 0, 3, 1 << 20, 1, 1, 1, 1}, {1, 2, 255, 1, 1 << 20, 1, 1, 1, 1}, {1, 2, 0, 1, 4, 1, 1, 1, 1},
                               {1, 1, 160, 3, 1 << 20, 0, 1, 1, 1}, {1, 1, 160, 3, 1 << 20, 1, 161, 1, 1}, {1, 1, 160, 3, 1 << 20, 1, 1, 0, 1},
                               {1, 1, 160, 3, 1 << 20, 1, 1, 2, 1}, {1, 1, 160, 3, 1 << 20, 1, 1, 1, 0}, {1, 2, 0, 1, 1 << 20, 1, 1, 2, 1}};
enum { NFORCE = sizeof(FORCES) / sizeof(FORCES[0]) };
static void set_force(FwdIn& in, const Force& f) {
  in.force = {f.white_fwd, f.cs_min_blocks, f.cs_min_dout, f.cs_max_dout, f.last_fuse, f.last_min_blocks, f.bwd_split, f.lik_fuse};
  for (int l = 0; l < in.L; ++l) in.layer[l].has_C = save_c_enabled(f.save_c, in.layer[l].Mp);      // (model_layout.hpp: the buffer exists where the policy may use it)
}
static long g_walked = 0;
static FwdRecord<Args> g_rec;
static void check(const FwdIn& in) {
  g_in = &in;
  const FwdPlan p = fwd_plan(in);
  check_against_legacy(in, p);
  check_invariants(in, p);
  check_record(in, p, g_rec);
  ++g_walked;
}
static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static bool coin(uint32_t one_in = 2) { return rnd(one_in) == 0; }

// every shape against sampled flags: Mp x D_in x D_out x (n, S) with layer 0's and the inner layers' row blocks at each threshold
static void walk_shapes() {
  g_case = "shapes:";
  for (int Mp : MPS) for (int Din : DINS) for (int Dout : DOUTS) for (int B : BLOCKS) for (int S : {1, 2, 3, 5}) for (int dn = -1; dn <= 1; ++dn)
  for (int at0 = 0; at0 < 2; ++at0) {      // the threshold met by the inner layers (S n rows) or by layer 0 (n rows)
    const int64_t n = (at0 ? (int64_t)B * 16 : (int64_t)B * 16 / S) + dn;
    if (n < 1 || (at0 && S > 2)) continue;
    for (int L = 1; L <= 5; ++L) for (int rep = 0; rep < 3; ++rep) {
      FwdIn in{};
      in.n = n; in.S = S; in.L = L;
      in.prepare = coin(); in.save = coin(); in.need_last_F = coin(4); in.lik_target = coin(); in.sample_w = coin(8); in.with_grad = coin(8) ? coin() : in.save;
      in.caller_z = rnd(1u << L);
      in.white = coin(4);
      const int lik = rnd(4);      // Gaussian twice as often: the route with the most decisions behind it
      in.lik_gaussian = lik <= 1; in.lik_elementwise = lik <= 2;
      in.grad_first = rnd(L); in.grad_q_only = coin(4); in.head_ok = coin(); in.overlap = coin(); in.timing = coin(16);
      const bool last1 = coin();      // the fused last layer exists for D_out = 1
      for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        in.layer[l] = FwdIn::Layer{Mp, Mp - (int)rnd(8), l == 0 ? Din : Dout, (last && last1) ? 1 : Dout, (int)rnd(2), coin(6) ? (int)rnd(3) : DSDGP_MEAN_ZERO,
                                   (last || !coin(6)) ? 0 : 2, coin(5), coin(), !coin(4), false, !coin(8)};
      }
      set_force(in, FORCES[coin() ? 0 : rnd(NFORCE)]);
      check(in);
    }
  }
}
// every flag against a few shapes: the call's kind, the likelihood, the gradient set, every subset of caller draws (L <= 3), every
// forward-side force setting, with both sides of the fused last layer's scope
static void walk_flags() {
  g_case = "flags:";
  const struct { int Mp; int64_t n; int S; } shapes[] = {{128, 200, 2}, {128, 1000, 20}, {512, 64, 4}, {32, 40, 3}};
  for (const auto& sh : shapes) for (int L = 1; L <= 5; ++L) for (uint32_t zs = 0; zs < (L <= 3 ? 1u << L : 2u); ++zs) for (int gfirst = 0; gfirst < L; ++gfirst)
  for (int q_only = 0; q_only < 2; ++q_only) for (int call = 0; call < 5; ++call) for (int white = 0; white < 2; ++white) for (int lik = 0; lik < 3; ++lik)
  for (int bits = 0; bits < 16; ++bits) for (int f = 0; f < NFORCE; ++f) {
    const bool corner = bits == 0 || bits == 15;
    if (f != 0 && !corner) continue;      // the force settings: with none and with all of the four bits below
    FwdIn in{};
    in.n = sh.n; in.S = sh.S; in.L = L; in.caller_z = (L <= 3) ? zs : (zs ? 0x15u : 0u);
    // propagate | value | gradient | saved forward pass | value with a sample of the last layer (no caller, planned all the same)
    in.prepare = call != 0; in.save = in.with_grad = call == 2 || call == 3; in.need_last_F = call == 0 || call == 4; in.lik_target = call == 1 || call == 2 || call == 4;
    in.white = white != 0; in.lik_gaussian = lik == 0; in.lik_elementwise = lik <= 1;
    in.grad_first = gfirst; in.grad_q_only = q_only != 0;
    in.sample_w = bits & 1; in.head_ok = (bits & 2) && sh.Mp <= 128; in.overlap = bits & 4; in.timing = false;
    for (int l = 0; l < L; ++l) {
      const bool last = l == L - 1;
      in.layer[l] = FwdIn::Layer{sh.Mp, sh.Mp - 3, 5, last ? 1 : 5, DSDGP_KERN_RBF, DSDGP_MEAN_ZERO, (!last && (bits & 8)) ? 2 : 0, false, true, true, false, true};
    }
    set_force(in, FORCES[f]);
    check(in);
    if (f == 0 && L >= 2 && corner) {      // out of the fused launch's scope one condition at a time
      FwdIn::Layer& v = in.layer[L - 1];
      const FwdIn::Layer keep = v;
      v.alg_g = false; check(in); v = keep;
      v.need_tpt = false; check(in); v = keep;
      v.gemm = true; check(in); v = keep;
      v.mean_kind = DSDGP_MEAN_LINEAR; check(in); v = keep;
      v.D_in = 17; check(in); v = keep;
      v.has_bpart = false; check(in); v = keep;
      in.timing = true; check(in); in.timing = false;
    }
  }
}

// ---- (c) pinned rows: the benchmark configurations (tools/bench_configs.py) and config 2's per-GPU shards, one training step each
// (minibatch gathered, draws from the seed, Adam in the tail).  The expected values were read off the library as it was before the plan
// existed — a print at the end of its forward loop — not computed by fwd_plan.  Per layer: 8-wave small launch, d_split, A, c_d, [X^T;1]
// kept, launch.
struct PinLayer { bool small8; int d_split; bool A, C, XT1; FwdLaunch launch; };
struct Pin {
  const char* name;
  int L, M, widths[5], dout_last; int64_t n; int S; bool multiclass;
  int gfirst; bool q_only;      // config 5's natural-gradient evaluation ahead of its Adam step
  bool head_ok, overlap;
  DrawsAt draws; bool draws_ahead; int head_nblk; bool adjoints_from_lik, lik_in_chain; int lik_nblocks;
  PinLayer layer[5];
};
static const FwdLaunch CH = LAUNCH_CHAIN, GE = LAUNCH_GEMM, WR = LAUNCH_WITH_REVERSE;
static const Pin PINS[] = {
    //                               L  M    widths            DY n    S  multiclass, pass   head   overlap | draws ahead blocks | adjoints from lik, in chain, blocks
    {"config 1 (M = 50, one layer)", 1, 50, {8}, 1, 100, 1, false, 0, false, true, false, DRAWS_HEAD, false, 0, false, false, 1,
     {{false, 1, true, false, true, CH}}},
    // layer 0 on the 8-wave small launch, four workgroups per row block; A and [X^T;1] kept, no c_d; the last layer runs with its reverse pass
    {"config 2 (M = 128, S = 20, 1000 rows)", 3, 128, {8, 8, 8}, 1, 1000, 20, false, 0, false, true, true, DRAWS_HEAD, true, 40, true, true, 1250,
     {{true, 4, true, false, true, CH}, {false, 1, true, false, true, CH}, {false, 1, true, false, true, WR}}},
    {"config 2, shard of 500 rows", 3, 128, {8, 8, 8}, 1, 500, 20, false, 0, false, true, true, DRAWS_HEAD, true, 20, true, true, 625,
     {{true, 4, true, false, true, CH}, {false, 1, true, false, true, CH}, {false, 1, true, false, true, WR}}},
    {"config 2, shard of 250 rows", 3, 128, {8, 8, 8}, 1, 250, 20, false, 0, false, true, true, DRAWS_HEAD, true, 10, true, true, 313,
     {{true, 4, true, false, true, CH}, {false, 1, true, false, true, CH}, {false, 1, true, false, true, WR}}},
    // 157 row blocks in the inner layers: they too take the 8-wave launch, layer 1 with three workgroups per row block
    {"config 2, shard of 125 rows", 3, 128, {8, 8, 8}, 1, 125, 20, false, 0, false, true, true, DRAWS_HEAD, true, 5, true, true, 157,
     {{true, 4, true, false, true, CH}, {true, 3, true, false, true, CH}, {true, 1, true, false, true, WR}}},
    {"config 3 (M = 256, five layers)", 5, 256, {9, 9, 9, 9, 9}, 1, 2000, 20, false, 0, false, false, true, DRAWS_SIDE, true, 0, true, true, 2500,
     {{true, 4, true, false, true, CH}, {true, 1, true, false, true, CH}, {true, 1, true, false, true, CH}, {true, 1, true, false, true, CH},
      {true, 1, true, false, true, WR}}},
    {"config 4 (M = 512, MultiClass, 512 rows)", 3, 512, {784, 30, 30}, 10, 512, 10, true, 0, false, false, true, DRAWS_SIDE, true, 0, false, false, 20,
     {{false, 4, true, true, true, GE}, {false, 3, true, true, true, GE}, {false, 2, true, true, true, GE}}},
    // the natural-gradient evaluation of the last layer's (q_mu, q_sqrt): the layers below keep nothing, the last one A alone
    {"config 5 (M = 1024, 125 rows), natural-gradient evaluation", 3, 1024, {8, 8, 8}, 1, 125, 50, false, 2, true, false, true, DRAWS_SIDE, true, 0, true, true, 98,
     {{false, 4, false, false, false, GE}, {false, 1, false, false, false, GE}, {false, 1, true, false, false, GE}}},
    {"config 5, Adam step", 3, 1024, {8, 8, 8}, 1, 125, 50, false, 0, false, false, true, DRAWS_SIDE, true, 0, true, true, 98,
     {{false, 4, true, true, true, GE}, {false, 1, true, true, true, GE}, {false, 1, true, true, true, GE}}},
};
static FwdIn pin_in(const Pin& c) {
  FwdIn in{};
  in.n = c.n; in.S = c.S; in.L = c.L;
  in.prepare = in.save = in.with_grad = in.lik_target = true;
  in.lik_gaussian = in.lik_elementwise = !c.multiclass;
  in.grad_first = c.gfirst; in.grad_q_only = c.q_only; in.head_ok = c.head_ok; in.overlap = c.overlap;
  const int Mp = pad_M(c.M);
  for (int l = 0; l < c.L; ++l) {
    const bool last = l == c.L - 1;
    const int D_out = last ? c.dout_last : c.widths[l + 1];
    const int64_t R = (l == 0) ? c.n : (int64_t)c.S * c.n;
    // model_layout.hpp: the algebraic dl/dKu assembly where the rows dwarf D_out Mp; q_sqrt^T for Mp > 256, the GEMM passes and the fused last layer
    const bool gemm = Mp >= 512;
    in.layer[l] = FwdIn::Layer{Mp, c.M, c.widths[l], D_out, DSDGP_KERN_RBF, DSDGP_MEAN_ZERO, 0, gemm, (int64_t)4 * D_out * Mp <= R,
                               Mp > 256 || (last && c.L >= 2 && layer_last_built(Mp, c.widths[l], D_out)), false, true};
  }
  set_force(in, FORCE_DEFAULT);
  return in;
}
static void pinned() {
  for (const Pin& c : PINS) {
    g_case = std::string("pinned, ") + c.name + ":";
    const FwdIn in = pin_in(c);
    check(in);
    const FwdPlan p = fwd_plan(in);
    REQUIRE(p.draws == c.draws && p.draws_ahead == c.draws_ahead && p.head_nblk == c.head_nblk, "draws %d ahead %d head blocks %d", p.draws, p.draws_ahead, p.head_nblk);
    REQUIRE(p.adjoints_from_lik == c.adjoints_from_lik && p.lik_in_chain == c.lik_in_chain && p.lik_nblocks == c.lik_nblocks, "adjoints_from_lik %d lik_in_chain %d blocks %d",
            p.adjoints_from_lik, p.lik_in_chain, p.lik_nblocks);
    for (int l = 0; l < c.L; ++l) {
      const FwdPlan::Layer& y = p.layer[l];
      const PinLayer& w = c.layer[l];
      const FwdIn::Layer& v = in.layer[l];
      REQUIRE(sm_small(v.Mp, ceil_div(y.Rin, 16), v.D_in, false) == w.small8 && y.d_split == w.d_split, "layer %d: 8-wave small launch %d, d_split %d", l,
              (int)sm_small(v.Mp, ceil_div(y.Rin, 16), v.D_in, false), y.d_split);
      REQUIRE(y.save_A == w.A && y.save_C == w.C && y.save_XT1 == w.XT1 && y.launch == w.launch, "layer %d: A %d C %d XT1 %d launch %d", l, y.save_A, y.save_C,
              y.save_XT1, y.launch);
      REQUIRE(!y.whitened && y.draw == (l == c.L - 1 ? DRAW_NONE : (c.draws_ahead ? DRAW_READY : DRAW_HERE)) && y.lik_epilogue == (l == c.L - 1 && c.lik_in_chain),
              "layer %d: whitened %d draw %d lik_epilogue %d", l, y.whitened, y.draw, y.lik_epilogue);
    }
  }
}

int main() {
  walk_shapes();
  walk_flags();
  pinned();
  printf("forward_check: %ld inputs walked, the plan equals the transcribed decisions and every invariant holds\n", g_walked);
  return 0;
}
