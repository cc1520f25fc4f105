// rt_control_policy.hip -- ControlPolicy on the device (control_policy.hpp): the gains and references, and the control input, of
// every instance at its own time.
#include <cmath>

#include "rt_context.hpp"
#include "control_policy.hpp"

using namespace rtoc;

static bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Both entry points: refusals, the grid times, one launch.  x == nullptr: rtoc_control_policy (out: the policy records), else
// rtoc_control_input (out: u)
static int run_policy(rtoc_ctx* c, double t0, const double* t, int per_instance, int N, const double* x, double* out, int count, int flags,
                      bool input) {
  CHECK_READY(c);
  if (!c->buf[RTOC_BUF_RIC].p || !c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (c->sto_on && !c->dt_current) return RTOC_ERR_NOT_READY;
  if (c->dims.nu < 1) return RTOC_ERR_BAD_ARG;   // no actuated joint: no policy (and no lanes per row in control_input_kernel)
  if (N < 1 || N > c->nstages - 1 || count < 1 || count > c->batch || (per_instance != 0 && per_instance != 1)) return RTOC_ERR_BAD_ARG;
  if (!t || !out || (input && !x) || (flags & ~RTOC_POLICY_DEVICE_PTRS) || !std::isfinite(t0)) return RTOC_ERR_BAD_ARG;
  const bool host = !(flags & RTOC_POLICY_DEVICE_PTRS);
  const int nv = c->dims.nv, nu = c->dims.nu, nq = config_dim(c);
  const size_t nt = per_instance ? (size_t)count : 1, nx = input ? (size_t)count * (nq + nv) : 0;
  const size_t nout = (size_t)count * (input ? nu : rtoc_control_policy_stride(nu));
  if (host && (!all_finite(t, nt) || !all_finite(x, nx))) return RTOC_ERR_BAD_ARG;

  // scratch that only grows: the first call of a context (or the first with an STO problem) allocates, later ones only launch
  HIP_TRY(c->d_policy_tg.grow(c->sto_on ? (size_t)c->batch * c->max_stages : (size_t)c->max_stages));
  auto a = view_args<PolicyArgs>(c);
  a.t = t, a.x = x, a.out = out;
  if (host) {
    const size_t cap_x = (size_t)c->batch * (nq + nv);
    HIP_TRY(c->d_policy_stage.grow((size_t)c->batch + cap_x + (size_t)c->batch * rtoc_control_policy_stride(nu)));
    double* d = c->d_policy_stage.p;
    HIP_TRY(hipMemcpyAsync(d, t, sizeof(double) * nt, hipMemcpyHostToDevice, c->stream));
    if (input) HIP_TRY(hipMemcpyAsync(d + c->batch, x, sizeof(double) * nx, hipMemcpyHostToDevice, c->stream));
    a.t = d, a.x = d + c->batch, a.out = d + c->batch + cap_x;
  }
  PolicyTimesArgs ta{};
  ta.grid = c->d_grid.p, ta.dt_inst = c->sto_on ? c->d_dt.p : nullptr, ta.t = c->d_policy_tg.p;
  ta.nstages = c->nstages, ta.count = count, ta.t0 = t0;
  hipLaunchKernelGGL(policy_times_kernel, dim3(((c->sto_on ? count : 1) + 63) / 64), dim3(64), 0, c->stream, ta);
  HIP_TRY(hipGetLastError());
  a.ric = c->buf[RTOC_BUF_RIC].p, a.tg = c->d_policy_tg.p;
  a.count = count, a.N = N;
  a.tg_per_instance = c->sto_on ? 1 : 0, a.t_per_instance = per_instance;
  a.nq = nq;
  if (input) hipLaunchKernelGGL(control_input_kernel, dim3(count), dim3(64), sizeof(double) * 2 * (size_t)nu, c->stream, a);
  else hipLaunchKernelGGL(control_policy_kernel, dim3(count), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  if (host) {
    HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(double) * nout, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return RTOC_OK;
}

int rtoc_control_policy(rtoc_ctx* c, double t0, const double* t, int per_instance, int N, double* out, int count, int flags) {
  return run_policy(c, t0, t, per_instance, N, nullptr, out, count, flags, false);
}

int rtoc_control_input(rtoc_ctx* c, double t0, const double* t, int per_instance, int N, const double* x, double* u, int count, int flags) {
  return run_policy(c, t0, t, per_instance, N, x, u, count, flags, true);
}
