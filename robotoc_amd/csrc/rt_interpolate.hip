// rt_interpolate.hip -- SolutionInterpolator on the device (solution_interpolate.hpp): store, interpolate, query, forget.
#include <cmath>

#include "rt_context.hpp"
#include "solution_interpolate.hpp"

using namespace rtoc;

// What both calls refuse ahead of anything else, and the contacts that pack the f / mu stacks: shapes with contact rows need the
// schedule of the grid in force (the masks) and the model (3 or 6 rows per contact, from its contact_type); an STO problem the
// time steps of the grid in force
static int interp_ready(rtoc_ctx* c, int* ncontacts, unsigned* six_rows) {
  *ncontacts = 0, *six_rows = 0u;
  if (c->sto_on && !c->dt_current) return RTOC_ERR_NOT_READY;
  if (c->dims.nf_max <= 0) return RTOC_OK;
  if (!c->h_model || !c->d_active.p || !c->active_current) return RTOC_ERR_NOT_READY;
  const rtoc_robot_model& m = c->h_model->m;
  *ncontacts = m.ncontacts;
  for (int k = 0; k < m.ncontacts; ++k)
    if (m.contact_type[k] == RTOC_CONTACT_SURFACE) *six_rows |= 1u << k;
  return RTOC_OK;
}

static int launch_times(rtoc_ctx* c, double t0, double* t, double* dt_out, int* type_out) {
  InterpTimesArgs a{};
  a.grid = c->d_grid.p, a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  a.t = t, a.dt_out = dt_out, a.type_out = type_out;
  a.nstages = c->nstages, a.batch = c->batch, a.t0 = t0;
  hipLaunchKernelGGL(interp_times_kernel, dim3(((c->sto_on ? c->batch : 1) + 63) / 64), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_solution_store(rtoc_ctx* c, double t0) {
  CHECK_READY(c);
  int ncontacts;
  unsigned six_rows;
  const int rc = interp_ready(c, &ncontacts, &six_rows);
  if (rc) return rc;
  if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
  if (!std::isfinite(t0)) return RTOC_ERR_BAD_ARG;
  const size_t cap = (size_t)c->batch * c->max_stages, n = (size_t)c->batch * c->nstages;
  HIP_TRY(c->d_isol.reserve(cap * c->L.sol.stride));
  HIP_TRY(c->d_isol_t.reserve(2 * cap));
  HIP_TRY(c->d_isol_type.reserve(c->max_stages));
  HIP_TRY(c->d_isol_mask.reserve(c->max_stages));
  c->isol_n = 0;   // until every copy is under way
  HIP_TRY(hipMemcpyAsync(c->d_isol.p, c->buf[RTOC_BUF_SOL].p, sizeof(double) * n * c->L.sol.stride, hipMemcpyDeviceToDevice, c->stream));
  if (ncontacts > 0)
    HIP_TRY(hipMemcpyAsync(c->d_isol_mask.p, c->d_active.p, sizeof(unsigned) * c->nstages, hipMemcpyDeviceToDevice, c->stream));
  const int lrc = launch_times(c, t0, c->d_isol_t.p, c->d_isol_t.p + cap, c->d_isol_type.p);
  if (lrc) return lrc;
  c->isol_n = c->nstages, c->isol_per_instance = c->sto_on ? 1 : 0;
  c->isol_ncontacts = ncontacts, c->isol_six_rows = six_rows;
  return RTOC_OK;
}

int rtoc_solution_interpolate(rtoc_ctx* c, double t0) {
  CHECK_READY(c);
  int ncontacts;
  unsigned six_rows;
  int rc = interp_ready(c, &ncontacts, &six_rows);
  if (rc) return rc;
  if (!std::isfinite(t0)) return RTOC_ERR_BAD_ARG;
  if (!c->isol_n) return RTOC_OK;   // if (!has_stored_sol_) return (:34)
  if (c->isol_n > c->max_stages || c->isol_ncontacts != ncontacts || c->isol_six_rows != six_rows) return RTOC_ERR_BAD_ARG;
  const size_t cap = (size_t)c->batch * c->max_stages;
  HIP_TRY(c->d_interp_t.reserve(cap));
  rc = ensure_buffer(c, RTOC_BUF_SOL);
  if (rc) return rc;
  rc = launch_times(c, t0, c->d_interp_t.p, nullptr, nullptr);
  if (rc) return rc;
  auto a = view_args<InterpArgs>(c);
  a.st.sol = c->d_isol.p, a.st.t = c->d_isol_t.p, a.st.dt = c->d_isol_t.p + cap;
  a.st.type = c->d_isol_type.p, a.st.mask = ncontacts > 0 ? c->d_isol_mask.p : nullptr;
  a.st.n = c->isol_n, a.st.per_instance = c->isol_per_instance;
  a.out = c->buf[RTOC_BUF_SOL].p;
  a.t = c->d_interp_t.p, a.t_per_instance = c->sto_on ? 1 : 0;
  a.ncontacts = ncontacts, a.six_rows = six_rows;
  if (ncontacts == 0) a.rv.active = nullptr;
  hipLaunchKernelGGL(solution_interpolate_kernel, dim3((unsigned)((size_t)c->batch * c->nstages)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  c->vals_fresh = 0;   // the pre-pass kinematics belong to the previous iterate
  return RTOC_OK;
}

int rtoc_solution_stored(const rtoc_ctx* c, int* nstages) {
  if (!c || !nstages) return RTOC_ERR_BAD_ARG;
  *nstages = c->isol_n;
  return RTOC_OK;
}

int rtoc_solution_forget(rtoc_ctx* c) {
  if (!c) return RTOC_ERR_BAD_ARG;
  c->isol_n = 0;
  return RTOC_OK;
}
