// line_search.hpp -- the line search on the device: the performance index of DirectMultipleShooting::evalOCP, the backtracking
// loops of LineSearch (filter method, merit backtracking) and the LineSearchFilter of every instance.  Runtime kernels (not
// per shape): rt_line_search.hip launches them and is the one unit that includes this header.
#pragma once
#include "device_utils.hpp"
#include "record_view.hpp"

namespace rtoc {

// ---- DirectMultipleShooting::evalOCP's performance index (line search) ---------------------------------------------
// What {Intermediate,Impact,Terminal}Stage::evalOCP accumulate per grid point (src/ocp/intermediate_stage.cpp:52-81,
// impact_stage.cpp:53-76, terminal_stage.cpp:51-66) and LineSearch::lineSearchFilterMethod reads (src/line_search/line_search.cpp:
// 56-83): cost (the value the cost kernel stored), cost_barrier = - barrier sum log(slack) of the active rows
// (pdipm.hxx:195-200), primal_feasibility = l1 norms of the rows' residuals, of [ID; C] (contact_dynamics_data.hpp:195-197) and
// of Fx, P (split_kkt_residual.hxx:109-115); the terminal grid point carries its cost only.  On records linearised and NOT yet
// condensed.  partial: [batch][nstages][2] = (cost + barrier, violation); the reduction adds them in grid order.
struct EvalOcpArgs {
  RecView rv;             // con == nullptr: neither box rows nor cone rows
  const double* costval;  // [batch][nstages]
  const rtoc_box_row* rows;
  double* partial;
  int nrows;
  ConeRows cone;
  double barrier;
};

static __global__ __launch_bounds__(64) void eval_ocp_kernel(EvalOcpArgs a) {
  const int lane = threadIdx.x;
  const int st = blockIdx.x, b = blockIdx.y;
  if (b >= a.rv.batch || st >= a.rv.nstages) return;
  const rtoc_record_layout &kl = a.rv.L.kkt, &cl = a.rv.L.cdd, &nl = a.rv.L.con;
  double viol = 0.0, bar = 0.0;
  auto l1 = [&](const double* p, int n) {
    for (int i = lane; i < n; i += 64) viol += fabs(p[i]);
  };
  const rtoc_grid g = a.rv.grid[st];
  const size_t rec = (size_t)b * a.rv.nstages + st;
  const bool terminal = g.type == RTOC_GRID_TERMINAL, impact = g.type == RTOC_GRID_IMPACT;
  if (!terminal) {
    const double* kr = a.rv.kkt_at(rec);
    const double* cr = a.rv.cdd_at(rec);
    l1(kr + kl.off[RTOC_KKT_FX], a.rv.L.nx);
    if (!impact && g.dims > 0) l1(kr + kl.off[RTOC_KKT_PRES], g.dims);
    l1(cr + cl.off[RTOC_CDD_IDC], a.rv.nv() + g.dimf);
    if (a.rv.con) {
      const double* nr = a.rv.con_at(rec);
      if (!impact)
        for (int r = lane; r < a.nrows; r += 64)
          if (g.time_stage >= a.rows[r].level) {
            viol += fabs(nr[nl.off[RTOC_CON_RESIDUAL] + r]);
            bar -= log(nr[nl.off[RTOC_CON_SLACK] + r]);
          }
      if (a.cone.contacts > 0 && (!impact || a.cone.impact)) {
        const int row0 = a.cone.row0, n = a.cone.rows * (g.dimf / a.cone.dim);
        for (int r = lane; r < n; r += 64) {
          viol += fabs(nr[nl.off[RTOC_CON_RESIDUAL] + row0 + r]);
          bar -= log(nr[nl.off[RTOC_CON_SLACK] + row0 + r]);
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) viol += __shfl_xor(viol, off, 64), bar += __shfl_xor(bar, off, 64);
  if (lane == 0) {
    a.partial[2 * rec] = a.costval[rec] + a.barrier * bar;
    a.partial[2 * rec + 1] = viol;
  }
}

// out: [2][batch] = cost + cost_barrier | primal_feasibility
static __global__ void eval_ocp_reduce_kernel(const double* partial, double* out, int nstages, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double c = 0.0, v = 0.0;
  for (int st = 0; st < nstages; ++st) c += partial[2 * ((size_t)b * nstages + st)], v += partial[2 * ((size_t)b * nstages + st) + 1];
  out[b] = c;
  out[batch + b] = v;
}

// ---- LineSearch::lineSearchFilterMethod's backtracking loop, per instance (line_search.cpp:56-83) ----
// alpha: the trial step of every instance; active: 1 while the instance is still backtracking.
struct LsArgs {
  double* steps;        // [batch][2] RTOC_BUF_STEP (in: max primal step; out: accepted step)
  double* trial_steps;  // [batch][2] = (alpha, 0): the trial iterate moves the primal variables and the slacks only
  double* alpha;
  int* active;
  const int* accepted;
  int* nactive;
  int batch;
  double rate, min_step;
};
static __global__ void ls_begin_kernel(LsArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  const double s = a.steps[2 * b];
  a.alpha[b] = s;
  const int on = s > a.min_step ? 1 : 0;   // while (primal_step_size > settings_.min_step_size)
  a.active[b] = on;
  a.trial_steps[2 * b] = on ? s : 0.0;
  a.trial_steps[2 * b + 1] = 0.0;
  if (on) atomicAdd(a.nactive, 1);
}
static __global__ void ls_advance_kernel(LsArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch || !a.active[b]) return;
  if (a.accepted[b]) {            // filter_.augment done by the filter kernel; return primal_step_size
    a.active[b] = 0;
    a.steps[2 * b] = a.alpha[b];
    return;
  }
  const double s = a.alpha[b] * a.rate;   // primal_step_size *= step_size_reduction_rate
  a.alpha[b] = s;
  if (s > a.min_step) {
    a.trial_steps[2 * b] = s;
    atomicAdd(a.nactive, 1);
  } else {                       // the loop ends without an accepted trial: the reduced step is returned as it is
    a.active[b] = 0;
    a.steps[2 * b] = s;
  }
}

// ---- LineSearch::meritBacktrackingLineSearch (line_search.cpp:87-128), per instance ----
// penaltyParam (:120-128): (1 + margin_rate) x the largest SplitSolution::lagrangeMultiplierLinfNorm over the grid
// (split_solution.cpp:126-134: lmd, gmm, beta, nu_passive of a floating base, mu of the active contact dimensions, xi of the active
// switching-constraint rows).  One wave per instance.
struct LsPenaltyArgs {
  RecView rv;
  double* penalty;   // [batch]
  double margin;
};
static __global__ __launch_bounds__(64) void ls_penalty_kernel(LsPenaltyArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= a.rv.batch) return;
  const rtoc_record_layout& sl = a.rv.L.sol;
  const int nv = a.rv.nv(), np = a.rv.L.dims.np;
  double m = 0.0;
  auto linf = [&](const double* p, int n) {
    for (int i = lane; i < n; i += 64) m = fmax(m, fabs(p[i]));
  };
  for (int st = 0; st < a.rv.nstages; ++st) {
    const rtoc_grid g = a.rv.grid[st];
    const double* s = a.rv.sol_at((size_t)b * a.rv.nstages + st);
    linf(s + sl.off[RTOC_SOL_LMD], nv);
    linf(s + sl.off[RTOC_SOL_GMM], nv);
    // (the terminal record too: SplitSolution::lagrangeMultiplierLinfNorm of s[N] takes every field, line_search.cpp:120-128 --
    //  beta, nu_passive are zero there unless the caller uploaded something else; the terminal stage has no contact forces, mu of
    //  s[N] is never written by the solver and stays out)
    linf(s + sl.off[RTOC_SOL_BETA], nv);
    if (np > 0) linf(s + sl.off[RTOC_SOL_NUP], np);
    if (g.type == RTOC_GRID_TERMINAL) continue;
    linf(s + sl.off[RTOC_SOL_MU], g.dimf);
    if (g.type != RTOC_GRID_IMPACT && g.switching_constraint) linf(s + sl.off[RTOC_SOL_XI], g.dims);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if (lane == 0) a.penalty[b] = m * (1.0 + a.margin);
}
// phase 0: every instance gets the trial step eps (the directional derivative's trial, :96-103);
// phase 1: dd = (merit(eps) - merit) / eps;
// phase 2: armijoCondition (:111-117) of the active instances' trial at step alpha -> accepted.
struct LsMeritArgs {
  const double* cur;      // [2][batch] cost + barrier | violation of the iterate
  const double* trial;    // [2][batch] of the trial iterate
  const double* penalty;  // [batch]
  double* dd;             // [batch] directional derivative of the merit function
  double* trial_steps;    // [batch][2]
  const double* alpha;    // [batch]
  const int* active;
  int* accepted;
  int batch, phase;
  double eps, armijo;
};
static __global__ void ls_merit_kernel(LsMeritArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.batch) return;
  if (a.phase == 0) {
    a.trial_steps[2 * b] = a.eps;
    a.trial_steps[2 * b + 1] = 0.0;
    return;
  }
  const double merit = a.cur[b] + a.penalty[b] * a.cur[a.batch + b];
  const double merit_trial = a.trial[b] + a.penalty[b] * a.trial[a.batch + b];
  if (a.phase == 1) {
    a.dd[b] = (1.0 / a.eps) * (merit_trial - merit);
    return;
  }
  a.accepted[b] = (a.active[b] && merit_trial < merit + a.armijo * a.alpha[b] * a.dd[b]) ? 1 : 0;
}

// ---- LineSearchFilter of every instance (src/line_search/line_search_filter.cpp) -------------------
struct FilterArgs {
  double* filt;      // [batch][CAP][2] (cost, violation)
  int* nfilt;        // [batch]
  const double* cost;
  const double* viol;
  const int* mask;   // may be nullptr
  int* accepted;
  int count, cap;
  double cost_rate, viol_rate;
  int seed_empty;    // 1: only instances whose filter is empty take part (line_search.cpp:58-62: seed it with the current iterate)
};

static __global__ void line_search_filter_kernel(FilterArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.count) return;
  if (a.mask && !a.mask[b]) {
    a.accepted[b] = 0;
    return;
  }
  double* f = a.filt + (size_t)b * a.cap * 2;
  int n = a.nfilt[b];
  if (a.seed_empty && n != 0) {
    a.accepted[b] = 0;
    return;
  }
  const double c = a.cost[b], v = a.viol[b];
  // isAccepted (:26-39): an empty filter accepts; otherwise ANY entry that the pair improves on
  bool ok = n == 0;
  for (int e = 0; e < n && !ok; ++e)
    ok = (c < f[2 * e] - a.cost_rate * f[2 * e + 1]) || (v < (1.0 - a.viol_rate) * f[2 * e + 1]);
  a.accepted[b] = ok ? 1 : 0;
  if (!ok) return;
  // augment (:42-60): erase the entries the new pair dominates, keep the order, append
  int w = 0;
  for (int e = 0; e < n; ++e) {
    const double ce = f[2 * e], ve = f[2 * e + 1];
    if (!(ce <= c && ve <= v)) {
      f[2 * w] = ce;
      f[2 * w + 1] = ve;
      ++w;
    }
  }
  if (w == a.cap) {  // full: drop the oldest
    for (int e = 1; e < w; ++e) {
      f[2 * (e - 1)] = f[2 * e];
      f[2 * (e - 1) + 1] = f[2 * e + 1];
    }
    --w;
  }
  f[2 * w] = c;
  f[2 * w + 1] = v;
  a.nfilt[b] = w + 1;
}

}  // namespace rtoc
