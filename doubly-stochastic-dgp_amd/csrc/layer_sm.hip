// Dispatch of the SVGP_Layer chain kernels (layer_sm_impl.hpp).  The instances are compiled in three parts
// (layer_sm_{fwd,bwd}_{a,b,c}.hip: padded inducing counts 32..112, 128..256, 320..1024, each direction on its own) so that they
// build in parallel.
#include <stdlib.h>

#include "layer.hpp"

int layer_fwd_sm_a(dsdgp_ctx*, const LayerFwdArgs&, int, int, int, int);
int layer_fwd_sm_b(dsdgp_ctx*, const LayerFwdArgs&, int, int, int, int);
int layer_fwd_sm_c(dsdgp_ctx*, const LayerFwdArgs&, int, int, int, int);
int layer_bwd_sm_a(dsdgp_ctx*, const LayerBwdArgs&, int, int, int, int);
int layer_bwd_sm_b(dsdgp_ctx*, const LayerBwdArgs&, int, int, int, int);
int layer_bwd_sm_c(dsdgp_ctx*, const LayerBwdArgs&, int, int, int, int);

// which instance a launch takes — waves per row block, the small-launch form: sm_small / sm_nw of chain_policy.hpp
int layer_fwd_sm_launch(dsdgp_ctx* ctx, const LayerFwdArgs& a, int Mp, int kern_kind, int white) {
  const int small = sm_small(Mp, ceil_div(a.Rin, 16), a.D_in, false);
  if (Mp < 128) return layer_fwd_sm_a(ctx, a, Mp, kern_kind, white, small);
  if (Mp <= 256) return layer_fwd_sm_b(ctx, a, Mp, kern_kind, white, small);
  return layer_fwd_sm_c(ctx, a, Mp, kern_kind, white, small);
}
int layer_bwd_sm_launch(dsdgp_ctx* ctx, const LayerBwdArgs& a, int Mp, int kern_kind, int white) {
  const int small = sm_small(Mp, ceil_div(a.ldA, 16), a.D_in, true);
  if (Mp < 128) return layer_bwd_sm_a(ctx, a, Mp, kern_kind, white, small);
  if (Mp <= 256) return layer_bwd_sm_b(ctx, a, Mp, kern_kind, white, small);
  return layer_bwd_sm_c(ctx, a, Mp, kern_kind, white, small);
}
