// rt_sweep.hip -- the Riccati recursion: the backward plan, the backward / forward / sweep launchers, the horizon scan,
// the unconstrained recursion and dynamics.
#include "rt_context.hpp"
#include "fxx_structure.hpp"

using namespace rtoc;

// ---- hot path ---------------------------------------------------------------------------
// RTOC_OPT_BACKWARD_SCAN: the scan covers grids without switching-time optimisation; others take the serial kernel
static bool grid_has_sto(const rtoc_ctx* c) {
  for (int i = 0; i < c->nstages; ++i)
    if (c->h_grid[i].sto || c->h_grid[i].sto_next) return true;
  return false;
}
// the backward recursion: every grid (with switching-time optimisation: matrix scan + serial vector pass, riccati_scan_sto.hpp)
static bool scan_applies(const rtoc_ctx* c) {
  if (!c->backward_scan || c->h_grid.empty()) return false;
  if (c->backward_scan == 2 && c->batch > RTOC_SCAN_AUTO_MAX_BATCH) return false;  // auto: latency regime only
  if (c->nstages > SCAN_STO_MAX_STAGES && grid_has_sto(c)) return false;            // the vector pass keeps the grid in LDS
  return true;
}
// the forward recursion as a prefix scan: grids without switching-time optimisation (the dts chain is not a fixed affine map)
static bool forward_scan_applies(const rtoc_ctx* c) { return scan_applies(c) && !grid_has_sto(c); }

// Backward recursion as a horizon scan (riccati_scan.hpp): elements, log2 combination levels, then the
// policies of all grid points at once by the tile-split backward kernel in its one-stage mode.
int rtoc::ensure_scan_buffers(rtoc_ctx* c) {
  const KernelSet* ks = c->ks;
  const size_t per = (size_t)c->batch * c->max_stages;
  for (int i = 0; i < 3; ++i) HIP_TRY(c->d_scan[i].reserve(per * (i < 2 ? ks->scan_elt_stride : ks->scan_ps_stride)));
  if (grid_has_sto(c)) HIP_TRY(c->d_scan_sto.reserve(per * ks->sto_scr_stride));  // (grids with STO only)
  return RTOC_OK;
}

// the arguments every backward launch shares (the register-resident and register-wide paths run only without
// RTOC_OPT_WRITEBACK_KKT: writeback is set on the tile-split and scan paths alone)
static BwdArgs bwd_args(const rtoc_ctx* c, int first, int end) {
  BwdArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.kkt_rw = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.grid = c->d_grid.p;
  a.status = c->d_status.p;
  a.prof = c->d_prof.p;
  a.nstages = c->nstages;
  a.batch = end;
  a.first = first;
  a.writeback = c->writeback;
  a.max_dts0 = c->max_dts0;
  return a;
}

static int launch_backward_scan(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  int rc0 = ensure_scan_buffers(c);
  if (rc0) return rc0;
  const int n = c->nstages, nb = end - first;
  ScanArgs s{};
  s.kkt = c->buf[RTOC_BUF_KKT].p;
  s.grid = c->d_grid.p;
  s.status = c->d_status.p;
  s.src = c->d_scan[1].p;
  s.dst = c->d_scan[0].p;
  s.ps = c->d_scan[2].p;
  s.nstages = n;
  s.batch = end;
  s.first = first;
  s.dist = 0;
  launch(ks->scan_elt, dim3(n, nb), stream, s);
  int cur = 0;
  for (int d = 1; d < n; d *= 2) {
    s.src = c->d_scan[cur].p;
    s.dst = c->d_scan[cur ^ 1].p;
    s.dist = d;
    launch(ks->scan_comb, dim3(n - d, nb, 2), stream, s);
    cur ^= 1;
  }
  BwdArgs a = bwd_args(c, first, end);
  a.prof = nullptr;
  a.scan_ps = c->d_scan[2].p;
  a.scan_ps_stride = ks->scan_ps_stride;
  a.scan_ps_soff = ks->scan_ps_soff;
  const bool sto = grid_has_sto(c);
  StoScanArgs t{};
  // Grids with switching-time optimisation: the bundles of the vector pass (everything of the vector recursion that does not depend
  // on the chain) are prepared by n - 1 more workgroups per instance of the SAME launch -- unless the policy workgroups write the
  // mutated Quu, lu back into the KKT records (RTOC_OPT_WRITEBACK_KKT), which the preparation reads: then it runs first, by itself.
  const bool ride = sto && !c->writeback && ks->sto_prep.lds <= p.kern->lds;
  if (sto) {
    t.kkt = c->buf[RTOC_BUF_KKT].p, t.ric = c->buf[RTOC_BUF_RIC].p, t.grid = c->d_grid.p, t.status = c->d_status.p;
    t.ps = c->d_scan[2].p, t.scr = c->d_scan_sto.p;
    t.nstages = n, t.batch = end, t.first = first, t.max_dts0 = c->max_dts0, t.prof = c->d_prof.p;
    t.kkt_rw = c->writeback ? c->buf[RTOC_BUF_KKT].p : nullptr;   // the policy workgroups have no s+: lu is written by the vector pass
    if (!ride) launch(ks->sto_prep, dim3(n - 1, nb), stream, t);
  }
  a.sto_scr = ride ? c->d_scan_sto.p : nullptr;
  launch(*p.kern, dim3(nb, ride ? 2 * n - 1 : n), stream, a);
  if (sto) launch(ks->sto_vec, dim3(nb), stream, t);   // s, k, m, the STO quantities
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// RTOC_OPT_FXX_STRUCTURE: may the structure-exploiting backward kernel run on the resident records?
static int check_fxx(rtoc_ctx* c) {
  HIP_TRY(c->d_fxx_flag.reserve(1));
  HIP_TRY(hipMemsetAsync(c->d_fxx_flag.p, 0, sizeof(int), c->stream));
  auto a = view_args<FxxCheckArgs>(c);
  a.flag = c->d_fxx_flag.p;
  hipLaunchKernelGGL(fxx_structure_kernel, dim3(c->batch * (c->nstages - 1)), dim3(64), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  int bad = 1;
  HIP_TRY(hipMemcpyAsync(&bad, c->d_fxx_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->fxx_state = bad ? 2 : 1;
  return RTOC_OK;
}

// The backward recursion of one public call: the horizon scan (RTOC_OPT_BACKWARD_SCAN), else (RTOC_OPT_BACKWARD_REGISTER) the
// register-resident kernel (riccati_backward_rv.hpp, one launch per horizon; on grids with switching-time optimisation its STO form,
// structured Fxx only), else on the iCub-size shapes the register-wide kernel (riccati_backward_rw.hpp, structured Fxx only; with 1
// on batches of more instances than CUs -- below that the tile-split kernel's four waves per instance finish a horizon sooner --,
// with 2 always), else the tile-split / role-split kernel.  The only code that checks the records (it synchronises) or resets
// fxx_state: the entry points call it once, before any capture, and hand the plan to the launchers.
int rtoc::plan_backward(rtoc_ctx* c, BwdPlan* out) {
  const KernelSet* ks = c->ks;
  // the register kernels: the default variant only (an explicit RTOC_OPT_BACKWARD_WAVES keeps its kernel)
  const bool reg = c->bwd_register && !c->h_grid.empty() && c->nstages >= 2 && c->nstages <= RV_MAX_STAGES && !c->writeback &&
                   c->bwd_variant == default_bwd_variant(ks);
  const bool sto = reg && grid_has_sto(c);
  const bool rw = reg && ks->bwd_rw && !sto && (c->bwd_register >= 2 || c->batch > c->num_cus);
  // the caller may have rewritten the records since the runtime last saw them (a bound buffer, or its pointer handed out)
  const bool rewritable = c->fxx_mode == 0 && (!c->buf[RTOC_BUF_KKT].owned || c->kkt_exposed);
  int rc = RTOC_OK;
  auto structured = [&]() {   // a structured kernel to choose, and the records have the structure
    if (!((ks->bwd_sa && c->bwd_variant == 3) || rw) || c->fxx_mode == 1) return false;
    if (c->fxx_mode == 2) return true;
    if (c->fxx_state == 0 && rc == RTOC_OK) rc = check_fxx(c);
    return c->fxx_state == 1;
  };
  BwdPlan p = {BWD_TILE, nullptr, 0};
  if (scan_applies(c)) {
    p = {BWD_SCAN, &ks->bwd[ks->scan_policy_variant], 0};
  } else if (reg && ks->bwd_rv && (!sto || (ks->bwd_rv_sto && structured()))) {
    p.path = BWD_RV;
    p.kern = sto ? &ks->bwd_rv_sto : (ks->bwd_rv_sa && structured()) ? &ks->bwd_rv_sa : &ks->bwd_rv;
    // a rewritable buffer may have changed since the check that chose the structured form: the kernel verifies as it goes
    p.check_fxx = (p.kern != &ks->bwd_rv && rewritable) ? 1 : 0;
  } else {
    // the register-wide kernel never loads the structured rows of Fxx, so it cannot verify them: check them for every call
    if (rw && rewritable) c->fxx_state = 0;
    const bool s = structured();
    p.path = (rw && s) ? BWD_RW : BWD_TILE;
    p.kern = (rw && s) ? &ks->bwd_rw : s ? &ks->bwd_sa : &ks->bwd[c->bwd_variant];
  }
  if (rc) return rc;
  // the plan is part of a captured graph: a new epoch when it changes, not whenever the records are checked again
  if (p.path != c->bwd_plan.path || p.kern != c->bwd_plan.kern || p.check_fxx != c->bwd_plan.check_fxx) c->epoch++;
  c->bwd_plan = *out = p;
  return RTOC_OK;
}

static int launch_backward_rv(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const int N = c->nstages - 1;
  BwdArgs a = bwd_args(c, first, end);
  // one launch for the whole horizon: regular, lift, impact and switching-constraint grid points are all the kernel's own
  a.seg_hi = N - 1;
  a.seg_lo = 0;
  a.check_fxx = p.check_fxx;
#ifdef RTOC_RV_DEBUG_MASK
  if (const char* e = getenv("RTOC_RV_DEBUG")) a.scan_ps_soff = atoi(e);
#endif
  if (N >= 1) launch(*p.kern, dim3(end - first), stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_rw(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  const int N = c->nstages - 1, nb = end - first;
  BwdArgs a = bwd_args(c, first, end);
  auto constrained = [&](int st) { return c->h_grid[st].type != RTOC_GRID_IMPACT && c->h_grid[st].dims > 0; };
  auto one_stage = [&](int st) {   // tile-split kernel, grid point st only (st == N: the terminal record)
    BwdArgs o = a;
    o.scan_ps = c->buf[RTOC_BUF_RIC].p + c->L.ric.off[RTOC_RIC_P];
    o.scan_ps_stride = c->L.ric.stride;
    o.scan_ps_soff = c->L.ric.off[RTOC_RIC_S] - c->L.ric.off[RTOC_RIC_P];
    o.seg_hi = o.seg_lo = st;
    launch(ks->bwd[ks->scan_policy_variant], dim3(nb, 1), stream, o);
  };
  if (N == 0 || constrained(N - 1)) one_stage(N);   // nobody else writes the terminal record then
  int hi = N - 1;
  while (hi >= 0) {
    if (constrained(hi)) {
      one_stage(hi);
      --hi;
      continue;
    }
    int lo = hi;
    while (lo > 0 && !constrained(lo - 1)) --lo;
    a.seg_hi = hi;
    a.seg_lo = lo;
    launch(*p.kern, dim3(nb), stream, a);
    hi = lo - 1;
  }
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_tile(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  launch(*p.kern, dim3((end - first + p.kern->inst - 1) / p.kern->inst), stream, bwd_args(c, first, end));
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_backward_range(rtoc_ctx* c, const BwdPlan& p, int first, int end, hipStream_t stream) {
  switch (p.path) {
    case BWD_SCAN: return launch_backward_scan(c, p, first, end, stream);
    case BWD_RV: return launch_backward_rv(c, p, first, end, stream);
    case BWD_RW: return launch_backward_rw(c, p, first, end, stream);
    default: return launch_backward_tile(c, p, first, end, stream);
  }
}
int rtoc::launch_backward(rtoc_ctx* c, const BwdPlan& p) { return launch_backward_range(c, p, 0, c->batch, c->stream); }

// Forward recursion as a prefix scan of the closed-loop maps (riccati_scan.hpp): maps of all grid points,
// log2 composition levels (dx of every grid point), then du / dlmdgmm / dxi of all grid points at once.
static int launch_forward_scan(rtoc_ctx* c, int first, int end, hipStream_t stream) {
  const KernelSet* ks = c->ks;
  int rc0 = ensure_scan_buffers(c);
  if (rc0) return rc0;
  const int n = c->nstages, nb = end - first, N = n - 1;
  FwdScanArgs s{};
  s.kkt = c->buf[RTOC_BUF_KKT].p;
  s.ric = c->buf[RTOC_BUF_RIC].p;
  s.dir = c->buf[RTOC_BUF_DIR].p;
  s.dx0 = c->buf[RTOC_BUF_DX0].p;
  s.grid = c->d_grid.p;
  s.src = c->d_scan[1].p;
  s.dst = c->d_scan[0].p;
  s.nstages = n;
  s.batch = end;
  s.first = first;
  s.dist = 0;
  launch(ks->fscan_elt, dim3(N, nb), stream, s);
  int cur = 0;
  for (int d = 1; d < N; d *= 2) {
    s.src = c->d_scan[cur].p;
    s.dst = c->d_scan[cur ^ 1].p;
    s.dist = d;
    launch(ks->fscan_comb, dim3(N - d, nb), stream, s);
    cur ^= 1;
  }
  launch(ks->fscan_fin, dim3(n, nb), stream, s);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

static int launch_forward_range(rtoc_ctx* c, int first, int end, hipStream_t stream) {
  if (forward_scan_applies(c)) return launch_forward_scan(c, first, end, stream);
  FwdArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.dx0 = c->buf[RTOC_BUF_DX0].p;
  a.grid = c->d_grid.p;
  a.nstages = c->nstages;
  a.batch = end;
  a.first = first;
  // (the kernel reads P from its lower triangle.  A structured-Fxx form -- rows [0, NV) of Fxx not read but for the two corners --
  // is not built: the bare pattern reads a matrix 11-12 % faster with the top halves silent, against 19 % for the triangle
  // (profiles/r11_symmetric_reads.txt); the row-walk kernel's 1.27 vs 1.28 ms for that form predates the row-pair lane map)
  launch(c->ks->fwd, dim3(end - first), stream, a, ((a.nstages + 3) & ~3) * (int)sizeof(int));  // grid table in LDS
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}
int rtoc::launch_forward(rtoc_ctx* c) { return launch_forward_range(c, 0, c->batch, c->stream); }

// Backward + forward sweep of the whole batch as a two-stream pipeline over instance chunks: the
// forward recursion of chunk i (HBM-bound, a few small waves per CU) runs under the backward
// recursion of chunk i+1 (MFMA / LDS-bound, leaves most of the HBM bandwidth idle).  Results are
// those of rtoc_riccati_backward followed by rtoc_riccati_forward.
int rtoc::launch_sweep(rtoc_ctx* c, const BwdPlan& p) {
  const int nch = (c->sweep_chunks > 0) ? c->sweep_chunks : 1;
  if (nch == 1 || p.path == BWD_SCAN) {  // the scan's element buffers are not chunked
    int rc = launch_backward(c, p);
    return rc ? rc : launch_forward(c);
  }
  const int per = (((c->batch + nch - 1) / nch) + 3) & ~3;  // whole 4-instance workgroups
  HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
  HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  for (int i = 0; i * per < c->batch; ++i) {
    const int first = i * per, end = (first + per < c->batch) ? first + per : c->batch;
    int rc = launch_backward_range(c, p, first, end, c->stream);
    if (rc) return rc;
    hipEvent_t e = c->ev_chunk[i % RTOC_MAX_CHUNK_EVENTS];
    HIP_TRY(hipEventRecord(e, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, e, 0));
    rc = launch_forward_range(c, first, end, c->stream2);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return RTOC_OK;
}

int rtoc_riccati_backward(rtoc_ctx* c) {
  CHECK_READY(c);
  BwdPlan p;
  int rc = plan_backward(c, &p);
  return rc ? rc : launch_backward(c, p);
}

int rtoc_riccati_forward(rtoc_ctx* c) {
  CHECK_READY(c);
  return launch_forward(c);
}

int rtoc_graph_replay_count(rtoc_ctx* c, unsigned long long* out) {
  if (!c || !out) return RTOC_ERR_BAD_ARG;
  *out = c->graph_replays;
  return RTOC_OK;
}

int rtoc_riccati_sweep(rtoc_ctx* c) {
  CHECK_READY(c);
  BwdPlan p;
  int rc = plan_backward(c, &p);
  return rc ? rc : run_graphed(c, &c->g_sweep, 0.0, 0.0, [&]() { return launch_sweep(c, p); });
}

static int launch_fill(rtoc_ctx* c, double dt) {
  FillArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.dt = dt;
  a.kl = c->L.kkt;
  launch(c->ks->fill, dim3(c->batch * c->nstages), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

// UnconstrRiccatiRecursion in its structured form (unconstr_riccati.hpp): whenever the shape has the kernels and the
// horizon scan is not asked for (the scan works on the general elements, i.e. on materialised A, B)
static bool unconstr_structured(const rtoc_ctx* c) {
  return c->ks->ubwd && c->dims.nf_max == 0 && !scan_applies(c) && !c->unconstr_dense;
}
static int launch_unconstr_riccati(rtoc_ctx* c, double dt, bool forward) {
  int rc = ensure_buffer(c, RTOC_BUF_RIC);
  if (!rc && forward) rc = ensure_buffer(c, RTOC_BUF_DIR);
  if (rc) return rc;
  if (!c->buf[RTOC_BUF_KKT].p) return RTOC_ERR_NOT_READY;
  UrArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.kkt_rw = c->buf[RTOC_BUF_KKT].p;
  a.ric = c->buf[RTOC_BUF_RIC].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.dx0 = c->buf[RTOC_BUF_DX0].p;
  a.status = c->d_status.p;
  a.nstages = c->nstages, a.batch = c->batch, a.writeback = c->writeback;
  a.dt = dt;
  a.kl = c->L.kkt, a.rl = c->L.ric, a.dl = c->L.dir;
  launch(forward ? c->ks->ufwd : c->ks->ubwd, dim3(c->batch), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_unconstr_backward(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (c->dims.nu != c->dims.nv || !(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (unconstr_structured(c)) return launch_unconstr_riccati(c, dt, false);
  BwdPlan p;
  int rc = launch_fill(c, dt);
  if (!rc) rc = plan_backward(c, &p);
  return rc ? rc : launch_backward(c, p);
}

static int launch_unconstr_dynamics(rtoc_ctx* c, bool expand, double dt) {
  if (c->dims.nu != c->dims.nv || c->dims.nf_max != 0) return RTOC_ERR_BAD_ARG;
  int rc = ensure_buffer(c, RTOC_BUF_CDD);
  if (rc) return rc;
  UdArgs a{};
  a.kkt = c->buf[RTOC_BUF_KKT].p;
  a.cdd = c->buf[RTOC_BUF_CDD].p;
  a.dir = c->buf[RTOC_BUF_DIR].p;
  a.nstages = c->nstages;
  a.batch = c->batch;
  a.nlin = dynamics_records(c);
  a.dt = dt;
  a.kl = c->L.kkt;
  a.cl = c->L.cdd;
  a.dl = c->L.dir;
  launch(expand ? c->ks->uexp : c->ks->ucond, dim3(c->batch * a.nlin), c->stream, a);
  HIP_TRY(hipGetLastError());
  return RTOC_OK;
}

int rtoc_unconstr_condense(rtoc_ctx* c) {
  CHECK_STAGES(c);
  return launch_unconstr_dynamics(c, false, 1.0);
}

int rtoc_unconstr_expand(rtoc_ctx* c, double dt) {
  CHECK_STAGES(c);
  if (!(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  return launch_unconstr_dynamics(c, true, dt);
}

int rtoc_unconstr_forward(rtoc_ctx* c, double dt) {
  CHECK_READY(c);
  if (c->dims.nu != c->dims.nv || !(dt > 0.0)) return RTOC_ERR_BAD_ARG;
  if (unconstr_structured(c)) return launch_unconstr_riccati(c, dt, true);
  return launch_forward(c);
}

int rtoc_check_fxx_structure(rtoc_ctx* c, int* structured) {
  CHECK_READY(c);
  int rc = check_fxx(c);
  if (rc) return rc;
  if (structured) *structured = c->fxx_state == 1;
  return RTOC_OK;
}
