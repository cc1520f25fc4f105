// rt_condense.hip -- condensation, expansion and update of the contact path: constraint rows, cones, state-equation correction.
#include "rt_context.hpp"
#include "pdipm_update.hpp"
#include "state_equation.hpp"

using namespace rtoc;

// RTOC_OPT_CONDENSE_REGISTER: the contact grid points by condense_rv_kernel (one wave per work item, products chained through
// registers), the impact grid points by condense_kernel.  Measured per 4096 ANYmal trot instances: 4.80 -> 4.00 ms without rows,
// 5.16 -> 4.55 ms with 72 joint-limit rows and 4 friction cones.
// friction cones of point contacts are condensed INSIDE condense_rv_kernel (their Gram product's tiles go straight into the seeds and
// operands of the condensation); wrench cones need their own kernel ahead of it
static bool cond_rv_fuses_cones(const rtoc_ctx* c) {
  return c->cone_contacts > 0 && c->cone_rows == RTOC_FRICTION_ROWS && c->cone_dim == 3 && c->ks->cond_fuses_cones && c->ks->cond_rv_cones;
}
static bool cond_register_applies(const rtoc_ctx* c) {
  if (!c->cond_register || !c->ks->cond_rv || c->condense_split || c->keep_qaf) return false;
  if (c->cone_contacts > 0 && !cond_rv_fuses_cones(c) && c->cond_register < 2) return false;
  return c->n_stage_contact + c->n_stage_impact == c->nstages - 1;
}

// The cone rows as the kernels see them (record_view.hpp): the one place their row numbers and record strides are worked out
ConeRows rtoc::view_cones(const rtoc_ctx* c) {
  ConeRows r{};
  r.dim = 3;
  if (c->cone_contacts <= 0) return r;
  r.contacts = c->cone_contacts, r.dim = c->cone_dim, r.rows = c->cone_rows;
  r.row0 = c->dims.nc_max - c->cone_rows * c->cone_contacts;
  r.stride = c->cone_rows == RTOC_WRENCH_ROWS ? rtoc_wrench_cone_stride(c->cone_contacts) : rtoc_cone_stride(c->dims.nv, c->cone_contacts);
  r.dgdf_off = rtoc_cone_dgdf_off(c->dims.nv, c->cone_contacts);
  r.impact = c->impact_cones;
  return r;
}

static int launch_condense(rtoc_ctx* c) {
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  CondArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.grid = c->d_grid.p;
  a.status = c->d_status.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.damping = c->contact_inv_damping;
  a.prof = c->d_prof.p;
  a.con = (c->nrows > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.rows = c->d_rows.p;
  a.entry = c->d_entry.p;
  a.pair = reinterpret_cast<const int4*>(c->d_pair.p);
  a.nrows = c->nrows;
  a.nl = c->L.con;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  const int nblocks = c->batch * (c->nstages - 1);
  a.keep_qaf = c->keep_qaf;
  a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  const bool rv = cond_register_applies(c);
  if ((rv ? cond_rv_fuses_cones(c) : (c->condense_split || c->ks->cond_fuses_cones)) && c->cone_contacts > 0) {  // the cone rows ride with the MJtJinv kernel / in wave 1 of the fused kernel / inside condense_rv_kernel
    if (!c->buf[RTOC_BUF_CONE].p || !c->buf[RTOC_BUF_CON].p) return RTOC_ERR_NOT_READY;
    const ConeRows cone = view_cones(c);
    a.cone_con = c->buf[RTOC_BUF_CON].p;
    a.cone = c->buf[RTOC_BUF_CONE].p;
    a.cone_rows = cone.rows, a.cone_contacts = cone.contacts, a.cone_dim = cone.dim, a.cone_row0 = cone.row0;
    a.cone_stride = cone.stride, a.cone_dgdf_off = cone.dgdf_off, a.cone_impact = cone.impact;
  }
  if (rv) {
    a.stage_list = c->d_stage_list.p;
    a.nlist = c->n_stage_contact;
#ifdef RTOC_CRV_DEBUG_LDS_PAD   // occupancy experiments (debug builds only): extra dynamic LDS per work item, clamped to what a launch accepts
    static const int lds_pad_env = getenv("RTOC_CRV_LDS_PAD") ? atoi(getenv("RTOC_CRV_LDS_PAD")) : 0;
    const int lds_room = 64 * 1024 - c->ks->cond_rv.lds;
    const int lds_pad = lds_pad_env < 0 ? 0 : (lds_pad_env > lds_room ? lds_room : lds_pad_env);
#else
    constexpr int lds_pad = 0;
#endif
    if (a.nlist > 0) {
      launch(a.cone_rows ? c->ks->cond_rv : c->ks->cond_rv_nc, dim3(c->batch * a.nlist), c->stream, a, lds_pad);
      HIP_TRY(hipGetLastError());
    }
    a.stage_list = c->d_stage_list.p + c->n_stage_contact;
    a.nlist = c->n_stage_impact;
    if (a.nlist > 0) launch(c->ks->cond, dim3(c->batch * a.nlist), c->stream, a);
  } else if (c->condense_split) {
    launch(c->ks->mjt, dim3(nblocks), c->stream, a);
    launch(c->ks->cond_split, dim3(nblocks), c->stream, a);
  } else {
    launch(c->ks->cond, dim3(nblocks), c->stream, a);
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// both step sizes of every instance back to 1 (RTOC_BUF_STEP), ahead of the kernels that take their minimum
void rtoc::launch_fill_steps(rtoc_ctx* c) {
  hipLaunchKernelGGL(fill_steps_kernel, dim3((2 * c->batch + 255) / 256), dim3(256), 0, c->stream, c->buf[RTOC_BUF_STEP].p, 2 * c->batch);
}

static int launch_expand(rtoc_ctx* c, double tau) {
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  ExpArgs a{};
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.cl = c->L.cdd;
  a.dl = c->L.dir;
  a.tau = tau;
  a.con = (c->nrows > 0) ? c->buf[RTOC_BUF_CON].p : nullptr;
  a.rows = c->d_rows.p;
  a.nrows = c->nrows;
  a.nl = c->L.con;
  a.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  a.dt_inst = c->sto_on ? c->d_dt.p : nullptr;
  a.prof = c->d_prof.p;
  launch_fill_steps(c);
  const int nblocks = c->batch * (c->nstages - 1);
  launch(c->ks->expd, dim3(nblocks), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_cones(rtoc_ctx* c, int phase, double tau) {  // 0 condense, 1 expand, 2 update
  if (!c->buf[RTOC_BUF_CONE].p || !c->buf[RTOC_BUF_CON].p) return RTOC_ERR_NOT_READY;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  const ConeRows cone = view_cones(c);
  ConeArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.con = c->buf[RTOC_BUF_CON].p;
  a.cone = c->buf[RTOC_BUF_CONE].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.grid = c->d_grid.p;
  a.steps = (unsigned long long*)c->buf[RTOC_BUF_STEP].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.max_contacts = cone.contacts, a.contact_dim = cone.dim, a.rows_per_contact = cone.rows, a.row0 = cone.row0;
  a.cone_stride = cone.stride, a.dgdf_off = cone.dgdf_off, a.impact_cones = cone.impact;
  const bool wrench = cone.rows == RTOC_WRENCH_ROWS;
  a.tau = tau;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  a.nl = c->L.con;
  a.dl = c->L.dir;
  const dim3 grid(c->batch * (c->nstages - 1));
  if (phase == 0)
    launch(wrench ? c->ks->wcond : c->ks->ccond, grid, c->stream, a);
  else if (phase == 1)
    launch(wrench ? c->ks->wexp : c->ks->cexp, grid, c->stream, a);
  else
    hipLaunchKernelGGL(cone_update_kernel, grid, dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_state_correction(rtoc_ctx* c, int mode) {
  if (!c->buf[RTOC_BUF_SE3].p) return RTOC_ERR_BAD_ARG;
  const auto a = view_args<SeArgs>(c);
  const int nblocks = (mode == 2) ? c->batch : c->batch * c->nstages;
  if (mode == 0)
    hipLaunchKernelGGL(state_correction_kernel<0>, dim3(nblocks), dim3(64), 0, c->stream, a);
  else if (mode == 1)
    hipLaunchKernelGGL(state_correction_kernel<1>, dim3(nblocks), dim3(64), 0, c->stream, a);
  else
    hipLaunchKernelGGL(state_correction_kernel<2>, dim3(nblocks), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_correct_state_equation(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;  // floating base only (hasFloatingBase())
  return launch_state_correction(c, 0);
}

int rtoc_correct_costate_direction(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  return launch_state_correction(c, 1);
}

int rtoc_compute_initial_state_direction(rtoc_ctx* c) {
  CHECK_READY(c);
  if (c->dims.np != 6) return RTOC_ERR_BAD_ARG;
  return launch_state_correction(c, 2);
}

int rtoc_condense(rtoc_ctx* c) {
  CHECK_READY(c);
  int rc = RTOC_OK;
  if (c->cone_contacts > 0 && (cond_register_applies(c) ? !cond_rv_fuses_cones(c) : (!c->condense_split && !c->ks->cond_fuses_cones)))
    rc = launch_cones(c, 0, 0.0);  // Constraints::condenseSlackAndDual first
  if (!rc) rc = launch_condense(c);
  if (!rc && c->buf[RTOC_BUF_SE3].p && c->dims.np == 6) rc = launch_state_correction(c, 0);
  return rc;
}

int rtoc_expand(rtoc_ctx* c, double tau) {
  CHECK_READY(c);
  if (!(tau > 0.0 && tau <= 1.0)) return RTOC_ERR_BAD_ARG;
  int rc = launch_expand(c, tau);
  if (!rc && c->cone_contacts > 0) rc = launch_cones(c, 1, tau);
  if (!rc && c->buf[RTOC_BUF_SE3].p && c->dims.np == 6) rc = launch_state_correction(c, 1);
  return rc;
}

int rtoc_update(rtoc_ctx* c) {
  CHECK_STAGES(c);
  if (c->cone_contacts > 0) {
    int rc = launch_cones(c, 2, 0.0);
    if (rc) return rc;
  }
  if (c->nrows == 0) return RTOC_OK;
  auto a = view_args<UpdArgs>(c);
  a.rows = c->d_rows.p, a.nrows = c->nrows;
  hipLaunchKernelGGL(pdipm_update_kernel, dim3(c->batch * a.rv.nlin()), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int set_cones(rtoc_ctx* c, int max_contacts, int contact_dim, int rows_per_contact, size_t stride) {
  if (!c || max_contacts < 0) return RTOC_ERR_BAD_ARG;
  if (max_contacts == 0) {
    if (c->cone_contacts > 0) c->epoch++;   // the cone kernels leave the captured launch sequence
    c->cone_contacts = 0;
    c->cone_rows = 0;
    return RTOC_OK;
  }
  if ((contact_dim != 3 && contact_dim != 6) || max_contacts * contact_dim > c->dims.nf_max ||
      c->nrows + rows_per_contact * max_contacts > c->dims.nc_max || rows_per_contact * max_contacts > 64)
    return RTOC_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const size_t need = (size_t)c->batch * c->max_stages * stride;
  if (c->want[RTOC_BUF_CONE] != need) c->buf[RTOC_BUF_CONE].release();
  c->want[RTOC_BUF_CONE] = need;
  int rc = ensure_buffer(c, RTOC_BUF_CONE);
  if (!rc) rc = ensure_buffer(c, RTOC_BUF_CON);
  if (rc) return rc;
  c->cone_contacts = max_contacts;
  c->cone_dim = contact_dim;
  c->cone_rows = rows_per_contact;
  c->epoch++;
  return RTOC_OK;
}

int rtoc_set_friction_cones(rtoc_ctx* c, int max_contacts, int contact_dim) {
  if (!c) return RTOC_ERR_BAD_ARG;
  return set_cones(c, max_contacts, contact_dim, RTOC_FRICTION_ROWS, rtoc_cone_stride(c->dims.nv, max_contacts));
}

int rtoc_set_wrench_cones(rtoc_ctx* c, int max_contacts) {
  if (!c) return RTOC_ERR_BAD_ARG;
  return set_cones(c, max_contacts, 6, RTOC_WRENCH_ROWS, rtoc_wrench_cone_stride(max_contacts));
}

int rtoc_wrench_cone_matrix(double X, double Y, double mu, double* out) {
  if (!out || !(X > 0.0) || !(Y > 0.0) || !(mu > 0.0)) return RTOC_ERR_BAD_ARG;  // ctor checks :19-26
  // Rows: unilaterality; four friction-pyramid faces; centre of pressure inside the sole (tau_x, tau_y);
  // eight yaw-torque bounds -- one per sign pattern (sx, sy, sz) of the f_x, f_y and tau_z coefficients.
  const double xymu = (X + Y) * mu;
  double row[RTOC_WRENCH_ROWS][6] = {{0, 0, -1, 0, 0, 0},   {-1, 0, -mu, 0, 0, 0}, {1, 0, -mu, 0, 0, 0},
                                     {0, -1, -mu, 0, 0, 0}, {0, 1, -mu, 0, 0, 0},  {0, 0, -Y, -1, 0, 0},
                                     {0, 0, -Y, 1, 0, 0},   {0, 0, -X, 0, -1, 0},  {0, 0, -X, 0, 1, 0}};
  // (sign of Y f_x, sign of X f_y) for rows 9..12; rows 13..16 mirror them with tau_z = +1
  static const int sg[4][2] = {{-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
  for (int i = 0; i < 4; ++i) {
    double* lo = row[9 + i];
    double* hi = row[13 + i];
    lo[0] = sg[i][0] * Y;  lo[1] = sg[i][1] * X;  lo[2] = -xymu;
    lo[3] = -sg[i][0] * mu; lo[4] = -sg[i][1] * mu; lo[5] = -1;
    hi[0] = -sg[i][0] * Y; hi[1] = -sg[i][1] * X; hi[2] = -xymu;
    hi[3] = -sg[i][0] * mu; hi[4] = -sg[i][1] * mu; hi[5] = 1;
  }
  for (int j = 0; j < RTOC_WRENCH_ROWS; ++j)
    for (int m = 0; m < 6; ++m) out[j + RTOC_WRENCH_ROWS * m] = row[j][m];
  return RTOC_OK;
}

int rtoc_set_constraint_rows(rtoc_ctx* c, const rtoc_box_row* rows, int nrows) {
  if (!c || nrows < 0 || nrows + c->cone_rows * c->cone_contacts > c->dims.nc_max || (nrows > 0 && !rows))
    return RTOC_ERR_BAD_ARG;
  for (int r = 0; r < nrows; ++r) {
    const rtoc_box_row& w = rows[r];
    const int lim = (w.var == RTOC_VAR_U) ? c->dims.nu : c->dims.nv;
    if (w.var < 0 || w.var > RTOC_VAR_A || w.index < 0 || w.index >= lim || (w.sign != 1 && w.sign != -1) ||
        w.level < 0 || w.level > 2)
      return RTOC_ERR_BAD_ARG;
    // acceleration limits are acceleration-level rows of the contact path (the unconstrained path has no `a` beside its control)
    if (w.var == RTOC_VAR_A && (w.level != 0 || c->dims.nf_max == 0)) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (nrows > 0) {
    int rc = ensure_buffer(c, RTOC_BUF_CON);
    if (rc) return rc;
    HIP_TRY(c->d_rows.reserve(c->dims.nc_max));
    HIP_TRY(hipMemcpyAsync(c->d_rows.p, rows, sizeof(rtoc_box_row) * nrows, hipMemcpyHostToDevice, c->stream));
    // rows grouped by the primal entry they act on (ascending row index inside a group, i.e. the
    // order in which the reference's components touch that entry)
    // primal entries: q (nv), v (nv), u (nu), a (nv)
    const int nv = c->dims.nv, ne = 3 * nv + c->dims.nu;
    std::vector<int> csr(ne + 1 + nrows, 0);
    auto entry_of = [&](const rtoc_box_row& w) {
      return w.var == RTOC_VAR_Q ? w.index : (w.var == RTOC_VAR_V ? nv + w.index : (w.var == RTOC_VAR_U ? 2 * nv + w.index : 2 * nv + c->dims.nu + w.index));
    };
    for (int r = 0; r < nrows; ++r) csr[entry_of(rows[r]) + 1]++;
    for (int e = 0; e < ne; ++e) csr[e + 1] += csr[e];
    std::vector<int> fill(csr.begin(), csr.begin() + ne);
    for (int r = 0; r < nrows; ++r) csr[ne + 1 + fill[entry_of(rows[r])]++] = r;
    HIP_TRY(c->d_entry.reserve(ne + 1 + c->dims.nc_max));
    HIP_TRY(hipMemcpyAsync(c->d_entry.p, csr.data(), sizeof(int) * csr.size(), hipMemcpyHostToDevice, c->stream));
    // the first two rows of every entry, packed (condense.hpp)
    std::vector<int> pair(4 * (size_t)ne, -1);
    for (int e = 0; e < ne; ++e)
      for (int k = 0; k < 2 && csr[e] + k < csr[e + 1]; ++k) {
        const int r = csr[ne + 1 + csr[e] + k];
        pair[4 * e + k] = r;
        pair[4 * e + 2 + k] = (rows[r].sign & 0xff) | (rows[r].level << 8);
      }
    HIP_TRY(c->d_pair.reserve(4 * ne));
    HIP_TRY(hipMemcpyAsync(c->d_pair.p, pair.data(), sizeof(int) * pair.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (nrows > 0) c->h_rows.assign(rows, rows + nrows);
  c->nrows = nrows;
  c->epoch++;
  return RTOC_OK;
}
