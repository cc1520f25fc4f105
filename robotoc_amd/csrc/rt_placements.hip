// rt_placements.hip -- the contact schedule and the desired contact placements of every instance (ModelState::cpos, crot): the
// setters and the getter, the forward kinematics to the contact frames (rtoc_contact_frame_placements) and the placements held
// where the feet are (rtoc_hold_contact_placements; contact_frame_placements.hpp).
#include <cmath>

#include "rt_context.hpp"
#include "contact_frame_placements.hpp"

using namespace rtoc;

// doubles of a placement table: the shared one is sized for any model, a per-instance one for the contacts of the model in force
static size_t placement_capacity(const rtoc_ctx* c, int per_instance, int unit) {
  return per_instance ? (size_t)c->batch * c->max_stages * c->h_model->m.ncontacts * unit : (size_t)c->max_stages * RTOC_MAX_CONTACTS * unit;
}
// The placements of the grid in force, staged, uploaded (the stream synchronised) and committed; nullptr: that table reads as
// zeros / identities from here on.  A new epoch where a launcher reads something else afterwards
static int upload_placements(rtoc_ctx* c, const double* positions, const double* rotations, int per_instance) {
  const size_t rows = (size_t)(per_instance ? c->batch : 1) * c->nstages * c->h_model->m.ncontacts;
  HIP_TRY(c->cpos.stage(positions ? placement_capacity(c, per_instance, 3) : 0));
  HIP_TRY(c->crot.stage(rotations ? placement_capacity(c, per_instance, 9) : 0));
  if (positions) HIP_TRY(hipMemcpyAsync(c->cpos.target(), positions, sizeof(double) * rows * 3, hipMemcpyHostToDevice, c->stream));
  if (rotations) HIP_TRY(hipMemcpyAsync(c->crot.target(), rotations, sizeof(double) * rows * 9, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  commit_rows(c, c->cpos, per_instance, positions != nullptr), commit_rows(c, c->crot, per_instance, rotations != nullptr);
  return RTOC_OK;
}

int rtoc_set_contact_schedule(rtoc_ctx* c, const unsigned* active, const double* positions, const double* rotations) {
  CHECK_READY(c);
  if (!c->h_model || !active) return RTOC_ERR_BAD_ARG;
  const rtoc_robot_model& m = c->h_model->m;
  const int nc = m.ncontacts;
  for (int i = 0; i < c->nstages; ++i) {
    if (nc < 32 && (active[i] >> nc) != 0) return RTOC_ERR_BAD_ARG;
    int rows = 0;
    for (int k = 0; k < nc; ++k)
      if ((active[i] >> k) & 1u) rows += m.contact_type[k] == RTOC_CONTACT_SURFACE ? 6 : 3;
    if (i < c->nstages - 1 && rows != c->h_grid[i].dimf) return RTOC_ERR_BAD_ARG;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(reserve_active(c));
  HIP_TRY(hipMemcpyAsync(c->d_active.p, active, sizeof(unsigned) * c->nstages, hipMemcpyHostToDevice, c->stream));
  const int rc = upload_placements(c, positions, rotations, 0);   // the batch shares these placements: a per-instance table ends here
  if (rc) return rc;
  c->h_active.assign(active, active + c->nstages);
  c->active_current = true;
  c->epoch++;   // the masks decide what the launchers do
  return RTOC_OK;
}

// a schedule that belongs to the grid in force, of a model with contacts
int rtoc::placements_ready(const rtoc_ctx* c) {
  if (!c->h_model || !c->d_active.p || !c->active_current || (int)c->h_active.size() != c->nstages) return RTOC_ERR_NOT_READY;
  return RTOC_OK;
}

int rtoc_set_contact_placements(rtoc_ctx* c, const double* positions, const double* rotations, int per_instance) {
  CHECK_READY(c);
  int rc = placements_ready(c);
  if (rc) return rc;
  if (per_instance != 0 && per_instance != 1) return RTOC_ERR_BAD_ARG;
  const int nc = c->h_model->m.ncontacts, ninst = per_instance ? c->batch : 1;
  if (nc < 1) return RTOC_ERR_BAD_ARG;
  // the entries of the ACTIVE contacts, the only ones a kernel reads, must be finite; the others are not looked at
  for (int b = 0; b < ninst; ++b)
    for (int i = 0; i < c->nstages; ++i)
      for (int k = 0; k < nc; ++k) {
        if (!((c->h_active[i] >> k) & 1u)) continue;
        const size_t row = ((size_t)b * c->nstages + i) * nc + k;
        for (int e = 0; positions && e < 3; ++e)
          if (!std::isfinite(positions[row * 3 + e])) return RTOC_ERR_BAD_ARG;
        for (int e = 0; rotations && e < 9; ++e)
          if (!std::isfinite(rotations[row * 9 + e])) return RTOC_ERR_BAD_ARG;
      }
  c->vals_fresh = 0;   // the contact rows of the values pre-pass belong to the previous placements
  return upload_placements(c, positions, rotations, per_instance);
}

int rtoc_get_contact_placements(rtoc_ctx* c, double* host_positions, double* host_rotations, int count, int* per_instance) {
  CHECK_READY(c);
  int rc = placements_ready(c);
  if (rc) return rc;
  if (count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  const size_t nc = c->h_model->m.ncontacts;
  if (per_instance) *per_instance = c->cpos.per_instance;
  // the table as an instance reads it: zeros / identities where nothing was set
  auto fetch = [&](double* host, const GridTable<double>& t, int unit) -> hipError_t {
    if (!host) return hipSuccess;
    if (t.on) return t.download(host, nc * unit, count, c->stream);
    for (size_t e = 0; e < (size_t)count * c->nstages * nc * unit; ++e) host[e] = (unit == 9 && (e % 9) % 4 == 0) ? 1.0 : 0.0;
    return hipSuccess;
  };
  HIP_TRY(fetch(host_positions, c->cpos, 3));
  HIP_TRY(fetch(host_rotations, c->crot, 9));
  return RTOC_OK;
}

// where the kinematics are evaluated: q of instance 0 and the doubles between two instances
static int placement_source(const rtoc_ctx* c, int source, int grid_point, const double** q, size_t* stride) {
  const rtoc_robot_model& m = c->h_model->m;
  if (source == 0) {
    if (!c->d_x0.p) return RTOC_ERR_NOT_READY;
    *q = c->d_x0.p, *stride = (size_t)m.nq + m.nv;
  } else if (source == 1) {
    if (grid_point < 0 || grid_point >= c->nstages) return RTOC_ERR_BAD_ARG;
    if (!c->buf[RTOC_BUF_SOL].p) return RTOC_ERR_NOT_READY;
    *q = c->buf[RTOC_BUF_SOL].p + (size_t)grid_point * c->L.sol.stride + c->L.sol.off[RTOC_SOL_Q];
    *stride = (size_t)c->nstages * c->L.sol.stride;
  } else {
    return RTOC_ERR_BAD_ARG;
  }
  return RTOC_OK;
}
static int launch_frame_placements(rtoc_ctx* c, FkArgs a) {
  a.rv = view(c);
  a.md = model_dims(c);
  const int G = 64 / a.md.gs;
  const size_t lds = sizeof(double) * G * (a.md.njoints + a.md.ncontacts) * FK_SLOTS;
  hipLaunchKernelGGL(contact_frame_placements_kernel, dim3((unsigned)((c->batch + G - 1) / G)), dim3(64), lds, c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_contact_frame_placements(rtoc_ctx* c, int source, int grid_point, double* host_R, double* host_p, double* host_com, int count) {
  CHECK_READY(c);
  if (count < 0 || count > c->batch) return RTOC_ERR_BAD_ARG;
  if (!c->h_model) return RTOC_ERR_NOT_READY;
  FkArgs a{};
  int rc = placement_source(c, source, grid_point, &a.q, &a.q_stride);
  if (rc) return rc;
  const size_t nc = c->h_model->m.ncontacts, B = c->batch;
  HIP_TRY(c->d_fk.reserve(B * (RTOC_MAX_CONTACTS * FK_SLOTS + 3)));
  a.out_R = c->d_fk.p, a.out_p = a.out_R + B * RTOC_MAX_CONTACTS * 9, a.out_com = a.out_p + B * RTOC_MAX_CONTACTS * 3;
  rc = launch_frame_placements(c, a);
  if (rc) return rc;
  if (host_R && nc > 0) HIP_TRY(hipMemcpyAsync(host_R, a.out_R, sizeof(double) * count * nc * 9, hipMemcpyDeviceToHost, c->stream));
  if (host_p && nc > 0) HIP_TRY(hipMemcpyAsync(host_p, a.out_p, sizeof(double) * count * nc * 3, hipMemcpyDeviceToHost, c->stream));
  if (host_com) HIP_TRY(hipMemcpyAsync(host_com, a.out_com, sizeof(double) * count * 3, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTOC_OK;
}

// A table per instance, every instance starting from what the batch shared (zeros / identities where nothing was set).  The
// shared rows are read while the new ones are written: never in place
int rtoc::placements_per_instance(rtoc_ctx* c, bool need_rot) {
  const int nc = c->h_model->m.ncontacts, inst = c->cpos.per_instance;
  const bool new_p = !(inst && c->cpos.on), new_r = c->crot.on ? !inst : need_rot;
  HIP_TRY(c->cpos.stage(new_p ? placement_capacity(c, 1, 3) : 0, false));
  HIP_TRY(c->crot.stage(new_r ? placement_capacity(c, 1, 9) : 0, false));
  const size_t per = (size_t)c->nstages * nc;
  auto spread = [&](double* dst, const double* src, int unit) {
    const size_t total = (size_t)c->batch * per * unit;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(placements_broadcast_kernel, dim3(blocks), dim3(256), 0, c->stream, dst, src, per * unit, total, unit);
  };
  if (new_p) spread(c->cpos.target(), inst ? nullptr : c->cpos.rows(), 3);
  if (new_r) spread(c->crot.target(), c->crot.rows(), 9);
  if (new_p || new_r) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));   // the shared tables are read before they are freed
    commit_rows(c, c->cpos, 1), commit_rows(c, c->crot, 1, c->crot.on || new_r);
  }
  return RTOC_OK;
}
// the kinematics at the q of rtoc_set_initial_state, or at q[batch] a q_stride apart (FkArgs::q takes any source), the result left on
// the device (rt_foot_steps.hip)
int rtoc::launch_frame_positions(rtoc_ctx* c, double* out_p, double* out_com, double* out_R, const double* q, size_t q_stride) {
  FkArgs a{};
  if (q) {
    a.q = q, a.q_stride = q_stride;
  } else {
    const int rc = placement_source(c, 0, 0, &a.q, &a.q_stride);
    if (rc) return rc;
  }
  a.out_p = out_p, a.out_com = out_com, a.out_R = out_R;
  return launch_frame_placements(c, a);
}

int rtoc_hold_contact_placements(rtoc_ctx* c, int source, int grid_point, int first, int last, unsigned contacts) {
  CHECK_READY(c);
  int rc = placements_ready(c);
  if (rc) return rc;
  const rtoc_robot_model& m = c->h_model->m;
  const int nc = m.ncontacts;
  if (nc < 1 || first < 0 || last > c->nstages || first >= last || (nc < 32 && (contacts >> nc) != 0)) return RTOC_ERR_BAD_ARG;
  FkArgs a{};
  rc = placement_source(c, source, grid_point, &a.q, &a.q_stride);
  if (rc) return rc;
  if (contacts == 0) return RTOC_OK;   // no foot on the ground: nothing to hold
  bool need_rot = false;
  for (int k = 0; k < nc; ++k)
    if (((contacts >> k) & 1u) && m.contact_type[k] == RTOC_CONTACT_SURFACE) need_rot = true;
  rc = placements_per_instance(c, need_rot);
  if (rc) return rc;
  a.tab_pos = c->cpos.rows(), a.tab_rot = c->crot.rows();
  a.first = first, a.last = last, a.contacts = contacts;
  c->vals_fresh = 0;
  return launch_frame_placements(c, a);
}
