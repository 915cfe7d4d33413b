// psi_front, the front end that the RBF kernel expectations (psi.hip, which defines it) share with their reverse pass (psi_grad.hip)
#pragma once
#include <math.h>
#include <functional>
#include <optional>

#include "common.hpp"
#include "psi_plan.hpp"

struct PsiFront {
  PsiPlan plan;
  char* base;                                      // the call's scratch
  double *ls2, *W1, *W2, *T, *H1, *H2, *Ltab;      // ls2: l_d^2, D entries (the reverse pass: l_d behind them); the tables of k_psi_rows / k_psi_cross
  std::optional<ProfScope> prof;                   // the call's profiler scope: opens before k_psi_rows, closes when the entry point returns
  double* at(const PsiRegion& r) const { return r.bytes ? (double*)(base + r.off) : nullptr; }
};
// Checks the arguments both calls share, then the caller's own (own_checks: nothing is launched before they pass), plans the forward call
// or (reverse) the reverse pass, takes the scratch, uploads the lengthscales and launches k_psi_rows and — want1 || want2 — k_psi_cross.
// psi1 goes to psi1 / ld1 in the forward call and to the plan's region A (n x M) in the reverse pass.
int psi_front(dsdgp_ctx* ctx, const dsdgp_kernel* kern, const double* Z, int32_t M, const double* mu, const double* s, int64_t n,
              bool reverse, bool want1, bool want2, bool want_dZ, const std::function<int()>& own_checks, const char* scope,
              double* psi0, double* psi1, int64_t ld1, PsiFront& F);
