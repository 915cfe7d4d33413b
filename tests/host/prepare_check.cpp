// Stand-alone check of the prepare plan (csrc/prepare_plan.hpp) on the CPU: a ledger of parameter versions, every event sequence up to
// DEPTH over every configuration, exit 1 with a message on the first violated invariant; then a table of sequences that pins what is
// redone.  Built and run by tests/test_prepare_plan_cpu.py (system C++ compiler, address + undefined sanitizers).
#include "prepare_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

enum { MAXL = 3, DEPTH = 5 };
static std::string g_case;      // a pinned row; empty: the walk is at g_path of g_cfg (put into words only when a check fails)
static std::string describe();
#define REQUIRE(cond, ...)                                                        \
  do {                                                                            \
    if (!(cond)) {                                                                \
      fprintf(stderr, "prepare_check: %s\n  violated: %s\n  ", describe().c_str(), #cond); \
      fprintf(stderr, __VA_ARGS__);                                               \
      fprintf(stderr, "\n");                                                      \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

// ---- configurations: the model as prepare_async sees it
struct Cfg { const char* name; int L; bool white; PrepIn in; PrepFactor route; };
static Cfg make_cfg(int L, bool white, int route, bool ext_ev) {
  static const char* names[] = {"head", "batched blocked", "per layer", "one-workgroup batch"};
  Cfg c{names[route], L, white, PrepIn{}, FACTOR_NONE};
  c.in.L = L; c.in.white = white; c.in.big_mp = 192; c.in.ext_ev = ext_ev;
  switch (route) {
    case 0: c.in.head_ok = true; c.in.mp_max = 32; c.route = FACTOR_IN_HEAD; break;
    case 1: c.in.uniform_big = true; c.in.blocked = (1u << L) - 1; c.in.mp_max = 192; c.route = FACTOR_BATCHED_BLOCKED; break;
    case 2: c.in.blocked = 1u; c.in.mp_max = 256; c.route = FACTOR_PER_LAYER; break;      // layer 0 blocked, the others one workgroup each
    default: c.in.mp_max = 160; c.route = FACTOR_ONE_WG_BATCH; break;
  }
  return c;
}

// ---- the ledger: versions of the two parts of every layer's parameters, and the versions every product was computed from
struct From { int kern, q; };
struct World {
  ParamState s;
  int kern[MAXL], q[MAXL];      // Z + kernel hyper-parameters | (q_mu, q_sqrt)
  int factor[MAXL];             // Lu, Lu^-1: the kern version they were computed from (-1: never)
  From trans[MAXL], fwd[MAXL], grad[MAXL];      // parameter transforms | forward side | gradient side: .kern is the FACTOR's version they read
  bool saved;                   // whether the saved pass stands, event by event: kept here independently of the record
  int64_t saved_n; int saved_S;
};
static World fresh(bool track) {
  World w{};
  for (int l = 0; l < MAXL; ++l) { w.factor[l] = -1; w.trans[l] = w.fwd[l] = w.grad[l] = From{-1, -1}; }
  if (track) w.s.set_track_theta(true);      // (as the Python engine does right after creating the model)
  return w;
}
static bool cur(const World& w, const From& f, int l) { return f.kern == w.kern[l] && f.q == w.q[l]; }
static bool factor_cur(const World& w, int l) { return w.factor[l] == w.kern[l]; }

// What must hold between any two calls, whatever came before
static void check_state(const World& w, const Cfg& c) {
  const ParamState& s = w.s;
  REQUIRE(s.saved == w.saved, "the record says saved = %d", (int)s.saved);
  REQUIRE(!s.saved || (s.saved_n == w.saved_n && s.saved_S == w.saved_S), "saved shape");
  REQUIRE(!s.saved || s.prepared, "a saved forward pass on a model that is not prepared");      // (backward_adjoints need not set `prepared`)
  const bool keep = s.track_theta && s.kuu_valid;
  for (int l = 0; l < c.L; ++l) {
    const bool mine = s.q == ParamState::Q_ONE && s.q_layer == l;      // the one layer whose q moved
    if (s.prepared) REQUIRE(factor_cur(w, l) && cur(w, w.trans[l], l) && cur(w, w.fwd[l], l), "prepared, layer %d stale (ensure_prepared would skip)", l);
    if (keep) REQUIRE(factor_cur(w, l), "the factor of layer %d would be kept and is stale", l);
    if (keep && s.q != ParamState::Q_UNKNOWN && !mine) {
      REQUIRE(cur(w, w.fwd[l], l), "the forward side of layer %d would be kept and is stale", l);
      if (s.prepared_grad && !c.white) REQUIRE(cur(w, w.grad[l], l), "the gradient side of layer %d would be kept and is stale", l);
    }
  }
}

// ---- events
static void ev_theta_moved(World& w, const Cfg& c) {
  for (int l = 0; l < c.L; ++l) { ++w.kern[l]; ++w.q[l]; }
  w.s.theta_moved();
  w.saved = false;
}
static void ev_q_moved(World& w, int l) { ++w.q[l]; w.s.q_moved(l); w.saved = false; }
static void ev_track(World& w, bool on) { w.s.set_track_theta(on); }
// prepare_async + what the plan says, applied to the ledger
// (`side` moves launches to the other stream and adds events, nothing else: both values are planned at every prepare, one is applied)
static PrepPlan plan_checked(const World& w, const Cfg& c, bool with_grad, int gfirst, bool side) {
  PrepIn in = c.in; in.with_grad = with_grad; in.grad_first = gfirst; in.side = side;
  const bool grad = with_grad && !c.white, track = w.s.track_theta;
  const PrepPlan p = prep_plan(w.s, in);
  // the plan is consistent in itself and with the model
  REQUIRE(p.head == in.head_ok && !(p.head && p.prep_kuu), "head %d prep_kuu %d", (int)p.head, (int)p.prep_kuu);
  REQUIRE(p.kuu_blocks == (p.prep_kuu && !p.keep_kuu), "Ku blocks %d, prep_kuu %d keep_kuu %d", (int)p.kuu_blocks, (int)p.prep_kuu, (int)p.keep_kuu);
  REQUIRE(p.factor == (p.head ? FACTOR_IN_HEAD : (p.keep_kuu ? FACTOR_NONE : c.route)), "factor route %d", (int)p.factor);
  REQUIRE(p.factor != FACTOR_PER_LAYER || p.blocked == in.blocked, "per-layer choice");
  REQUIRE(p.keep_kuu || p.head || p.prep_kuu, "a new factor of a Ku nobody rebuilt");
  REQUIRE(p.fwd != REDO_FROM && (p.fwd != REDO_LAYER || (p.fwd_layer >= 0 && p.fwd_layer < c.L)), "forward side: %d, layer %d", (int)p.fwd, p.fwd_layer);
  REQUIRE(grad || p.grad == REDO_NONE, "gradient side without a gradient / on a white model");
  REQUIRE((p.grad != REDO_LAYER && p.grad != REDO_FROM) || (p.grad_layer >= 0 && p.grad_layer < c.L), "gradient side: layer %d", p.grad_layer);
  // events
  REQUIRE(p.fork_on_head == (in.head_ok && side && in.ext_ev), "fork event on the head launch");
  REQUIRE(p.fork == (side && !p.early) && p.rec_prep_side == (side && !p.early), "fork %d, ev_prep_side %d", (int)p.fork, (int)p.rec_prep_side);
  REQUIRE(p.rec_kinv == (side && grad && !p.early), "ev_kinv %d", (int)p.rec_kinv);
  // with track_theta off nothing is ever reused
  if (!track)
    REQUIRE(!p.keep_kuu && !p.early && p.fwd == REDO_ALL && p.grad == (!grad ? REDO_NONE : (gfirst > 0 ? REDO_FROM : REDO_ALL)) &&
            (p.grad != REDO_FROM || p.grad_layer == gfirst), "track_theta is off and something is reused");
  // returns early: nothing was stale, nothing but the head launch runs
  if (p.early) {
    REQUIRE(!p.prep_kuu && (p.factor == FACTOR_NONE || p.factor == FACTOR_IN_HEAD) && p.keep_kuu && p.fwd == REDO_NONE && p.grad == REDO_NONE, "early return with work");
    for (int l = 0; l < c.L; ++l) {
      REQUIRE(factor_cur(w, l) && cur(w, w.fwd[l], l), "early return, layer %d stale", l);
      REQUIRE(!grad || cur(w, w.grad[l], l), "early return, gradient side of layer %d stale", l);
    }
  }
  return p;
}
static PrepPlan ev_prepare(World& w, const Cfg& c, bool with_grad, int gfirst) {
  w.s.workspace_overwritten(); w.saved = false;
  const bool grad = with_grad && !c.white;
  const PrepPlan p = plan_checked(w, c, with_grad, gfirst, false), ps = plan_checked(w, c, with_grad, gfirst, true);
  REQUIRE(p.head == ps.head && p.keep_kuu == ps.keep_kuu && p.prep_kuu == ps.prep_kuu && p.kuu_blocks == ps.kuu_blocks && p.factor == ps.factor &&
          p.early == ps.early && p.fwd == ps.fwd && p.fwd_layer == ps.fwd_layer && p.grad == ps.grad && p.grad_layer == ps.grad_layer &&
          p.grad_all == ps.grad_all, "the side stream changes what is redone");
  // apply
  for (int l = 0; l < c.L; ++l) {
    if (!p.keep_kuu) w.factor[l] = w.kern[l];
    if (p.head || p.prep_kuu) w.trans[l] = From{w.kern[l], w.q[l]};
    if (p.fwd == REDO_ALL || (p.fwd == REDO_LAYER && l == p.fwd_layer)) w.fwd[l] = From{w.factor[l], w.q[l]};
    if (p.grad == REDO_ALL || (p.grad == REDO_LAYER && l == p.grad_layer) || (p.grad == REDO_FROM && l >= p.grad_layer)) w.grad[l] = From{w.factor[l], w.q[l]};
  }
  w.s.prepare_done(p);
  // after any prepare
  for (int l = 0; l < c.L; ++l) {
    REQUIRE(factor_cur(w, l), "after prepare: factor of layer %d stale", l);
    REQUIRE(p.early || cur(w, w.trans[l], l), "after prepare: transforms of layer %d stale", l);
    REQUIRE(cur(w, w.fwd[l], l), "after prepare: forward side of layer %d stale", l);
    if (grad && l >= gfirst) REQUIRE(cur(w, w.grad[l], l), "after prepare: gradient side of layer %d stale", l);
    if (w.s.prepared_grad && !c.white) REQUIRE(cur(w, w.grad[l], l), "prepared_grad, gradient side of layer %d stale", l);
  }
  REQUIRE(w.s.prepared && w.s.kuu_valid && w.s.q == ParamState::Q_NONE, "after prepare: the record");
  return p;
}
// an evaluation: dsdgp_model_elbo
static PrepPlan ev_eval(World& w, const Cfg& c, bool with_grad, int gfirst) {
  const PrepPlan p = ev_prepare(w, c, with_grad, gfirst);
  w.s.workspace_overwritten();      // forward_layers
  if (with_grad) {
    w.s.grad_evaluated(pass_is_pruned(c.white, gfirst, false));
    REQUIRE(w.s.grad_pruned == (!c.white && gfirst > 0), "grad_pruned");
  }
  return p;
}
// dsdgp_model_forward_saved / dsdgp_model_backward_adjoints (refused unless the saved pass stands)
static void ev_saved(World& w, const Cfg& c) {
  ev_prepare(w, c, true, 0);
  w.s.workspace_overwritten();
  w.s.saved_recorded(40, 2);
  w.saved = true; w.saved_n = 40; w.saved_S = 2;
}
static void ev_consume(World& w) {
  if (!w.s.saved) return;
  w.s.saved_consumed(); w.saved = false;
  w.s.grad_evaluated(false);
}
// ensure_prepared of an entry point that leaves the workspace alone (dsdgp_model_layer_kl) -> whether it prepared
static bool ev_ensure(World& w, const Cfg& c) {
  if (w.s.prepared) return false;
  ev_prepare(w, c, false, 0);
  return true;
}

struct Event { char kind; int a, b; };      // T theta | Q q of layer a | K track a | E eval(with_grad a, grad_first b) | S saved | C consume | N ensure
static std::string name(const Event& e) {
  char t[64];
  switch (e.kind) {
    case 'T': return "theta moved";
    case 'Q': snprintf(t, sizeof t, "q of layer %d moved", e.a); return t;
    case 'K': return e.a ? "track on" : "track off";
    case 'E': snprintf(t, sizeof t, "%s(grad_first %d)", e.a ? "G" : "V", e.b); return t;
    case 'S': return "saved forward";
    case 'C': return "backward_adjoints";
    default: return "ensure_prepared";
  }
}
static void apply(World& w, const Cfg& c, const Event& e) {
  switch (e.kind) {
    case 'T': ev_theta_moved(w, c); break;
    case 'Q': ev_q_moved(w, e.a); break;
    case 'K': ev_track(w, e.a != 0); break;
    case 'E': ev_eval(w, c, e.a != 0, e.b); break;
    case 'S': ev_saved(w, c); break;
    case 'C': ev_consume(w); break;
    default: ev_ensure(w, c); break;
  }
  check_state(w, c);
}
static const Cfg* g_cfg;
static bool g_track;
static Event g_path[DEPTH];
static int g_len;
static std::string describe() {
  if (!g_case.empty()) return g_case;
  std::string t = std::string(g_cfg->name) + (g_cfg->white ? ", white" : "") + ", L = " + std::to_string(g_cfg->L) + (g_track ? ": (track on)" : ": (fresh)");
  for (int i = 0; i < g_len; ++i) t += " ; " + name(g_path[i]);
  return t;
}
static long walk(const World& w, const Cfg& c, const std::vector<Event>& events, int depth) {
  long n = 0;
  for (const Event& e : events) {
    g_path[g_len++] = e;
    World next = w;
    apply(next, c, e);
    n += 1 + (depth > 1 ? walk(next, c, events, depth - 1) : 0);
    --g_len;
  }
  return n;
}

// ---- pinned minimality: the last plan of a sequence.  Every row is written out by hand from the rules as DESIGN.md 5.7 and the
// comments of prepare_plan.hpp state them, not computed: the invariants above would accept "always redo everything"
struct Want { bool early, keep_kuu, prep_kuu, kuu_blocks; bool factor; PrepRedo fwd; int fwd_layer; PrepRedo grad; int grad_layer; bool grad_all; };
struct Row { const char* what; std::vector<Event> seq; Want head, plain; };      // on the head route | on the one-workgroup batch
static const Event V{'E', 0, 0}, G{'E', 1, 0}, T{'T', 0, 0};
static Event Gp(int first) { return Event{'E', 1, first}; }
static Event nat(int l) { return Event{'Q', l, 0}; }
static void pinned(const Cfg& c, bool head) {
  const PrepRedo NO = REDO_NONE, ONE = REDO_LAYER, FROM = REDO_FROM, ALL = REDO_ALL;
  //                       early keep prep  kuu   factor fwd     grad     prepared_grad
  const Row rows[] = {
    {"first evaluation: everything", {V},
      {false, false, false, false, true, ALL, 0, NO, 0, false}, {false, false, true, true, true, ALL, 0, NO, 0, false}},
    {"V then V at unchanged parameters: nothing but the head launch", {V, V},
      {true, true, false, false, false, NO, 0, NO, 0, false}, {true, true, false, false, false, NO, 0, NO, 0, false}},
    // (k_prep_kuu's parameter transforms run again here although nothing moved)
    {"G after V at unchanged parameters: gradient side only", {V, G},
      {false, true, false, false, false, NO, 0, ALL, 0, true}, {false, true, true, false, false, NO, 0, ALL, 0, true}},
    {"G then V at unchanged parameters: nothing (prepared_grad stands)", {G, V},
      {true, true, false, false, false, NO, 0, NO, 0, false}, {true, true, false, false, false, NO, 0, NO, 0, false}},
    {"G after a natgrad step on layer 2 alone: both sides of layer 2, no factor", {G, nat(2), G},
      {false, true, false, false, false, ONE, 2, ONE, 2, true}, {false, true, true, false, false, ONE, 2, ONE, 2, true}},
    {"V after a natgrad step on layer 2 alone: forward side of layer 2, no factor", {G, nat(2), V},
      {false, true, false, false, false, ONE, 2, NO, 0, false}, {false, true, true, false, false, ONE, 2, NO, 0, false}},
    {"pruned G after a natgrad step on layer 2: both sides of layer 2", {G, nat(2), Gp(2)},
      {false, true, false, false, false, ONE, 2, ONE, 2, false}, {false, true, true, false, false, ONE, 2, ONE, 2, false}},
    {"full G after a pruned natgrad evaluation: gradient side of all layers, forward side of layer 2 only", {G, nat(2), Gp(2), nat(2), G},
      {false, true, false, false, false, ONE, 2, ALL, 0, true}, {false, true, true, false, false, ONE, 2, ALL, 0, true}},
    {"natgrad steps on two layers: forward side of all layers, no factor", {G, nat(2), nat(0), V},
      {false, true, false, false, false, ALL, 0, NO, 0, false}, {false, true, true, false, false, ALL, 0, NO, 0, false}},
    {"after theta moved: everything", {G, T, G},
      {false, false, false, false, true, ALL, 0, ALL, 0, true}, {false, false, true, true, true, ALL, 0, ALL, 0, true}},
    {"pruned G after V at unchanged parameters: gradient side from layer 1", {V, Gp(1)},
      {false, true, false, false, false, NO, 0, FROM, 1, false}, {false, true, true, false, false, NO, 0, FROM, 1, false}},
    // two rules that redo more than is stale, pinned as they are:
    {"pruned G from layer 1 after a natgrad step on layer 0: the gradient side of layer 0 (which that pass does not read)", {G, nat(0), Gp(1)},
      {false, true, false, false, false, ONE, 0, ONE, 0, false}, {false, true, true, false, false, ONE, 0, ONE, 0, false}},
    {"... and the full G behind it redoes the gradient side of all layers (prepared_grad was dropped, every layer is current)", {G, nat(0), Gp(1), G},
      {false, true, false, false, false, NO, 0, ALL, 0, true}, {false, true, true, false, false, NO, 0, ALL, 0, true}},
  };
  for (const Row& r : rows) {
    g_case = std::string("pinned, ") + c.name + ": " + r.what;
    World w = fresh(true);
    PrepPlan p{};
    for (const Event& e : r.seq) {
      if (e.kind == 'E') p = ev_eval(w, c, e.a != 0, e.b);
      else apply(w, c, e);
      check_state(w, c);
    }
    const Want& x = head ? r.head : r.plain;
    REQUIRE(p.head == head && p.early == x.early && p.keep_kuu == x.keep_kuu && p.prep_kuu == x.prep_kuu && p.kuu_blocks == x.kuu_blocks,
            "early %d keep_kuu %d prep_kuu %d Ku blocks %d", (int)p.early, (int)p.keep_kuu, (int)p.prep_kuu, (int)p.kuu_blocks);
    REQUIRE((head ? !p.keep_kuu : p.factor != FACTOR_NONE) == x.factor, "factor route %d, keep_kuu %d", (int)p.factor, (int)p.keep_kuu);
    REQUIRE(p.fwd == x.fwd && (p.fwd != ONE || p.fwd_layer == x.fwd_layer), "forward side %d of layer %d", (int)p.fwd, p.fwd_layer);
    REQUIRE(p.grad == x.grad && ((p.grad != ONE && p.grad != FROM) || p.grad_layer == x.grad_layer), "gradient side %d of layer %d", (int)p.grad,
            p.grad_layer);
    REQUIRE(p.early || w.s.prepared_grad == x.grad_all, "prepared_grad %d", (int)w.s.prepared_grad);
  }
  // rules of the record itself
  g_case = "pinned: track switched off leaves `prepared` standing (theta did not move)";
  World w = fresh(true);
  ev_eval(w, c, false, 0);
  ev_track(w, false);
  REQUIRE(!ev_ensure(w, c), "ensure_prepared prepared again");
  g_case = "pinned: track off, V then V: everything again";
  const PrepPlan p = ev_eval(w, c, false, 0);
  REQUIRE(!p.early && !p.keep_kuu && p.fwd == ALL, "something was kept");
  g_case = "pinned: a natgrad step drops `prepared` and the saved pass, a switch of track_theta neither";
  w = fresh(true);
  ev_saved(w, c);
  ev_track(w, true);
  REQUIRE(w.s.saved && w.s.prepared && !w.s.kuu_valid, "after the switch");
  ev_saved(w, c);
  ev_q_moved(w, 1);
  REQUIRE(!w.s.saved && !w.s.prepared && w.s.kuu_valid, "after the step: saved %d prepared %d kuu_valid %d", (int)w.s.saved, (int)w.s.prepared, (int)w.s.kuu_valid);
}

int main() {
  long pairs = 0, configs = 0;
  for (int L = 1; L <= MAXL; ++L) for (int white = 0; white < 2; ++white) for (int route = 0; route < 4; ++route)
  for (int ext_ev = (route == 0 ? 0 : 1); ext_ev < 2; ++ext_ev) {      // ext_ev matters on the head route only
    const Cfg c = make_cfg(L, white != 0, route, ext_ev != 0);
    std::vector<Event> events{T, Event{'K', 0, 0}, Event{'K', 1, 0}, Event{'S', 0, 0}, Event{'C', 0, 0}, Event{'N', 0, 0}, V};
    for (int l = 0; l < L; ++l) { events.push_back(nat(l)); events.push_back(Gp(l)); }
    g_cfg = &c;
    for (int track = 0; track < 2; ++track) {
      g_track = track != 0;
      pairs += walk(fresh(g_track), c, events, DEPTH);
    }
    ++configs;
  }
  pinned(make_cfg(3, false, 0, true), true);
  pinned(make_cfg(3, false, 3, true), false);
  printf("prepare_check: %ld (sequence, configuration) pairs over %ld configurations, every invariant holds\n", pairs, configs);
  return 0;
}
