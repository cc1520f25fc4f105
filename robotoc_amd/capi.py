"""ctypes binding of the C ABI (include/rtoc.h) -- the same entry points a C++ host
or the reference's solver classes would bind.  There is NO CPU fallback: if
librtoc_hip.so is missing or no HIP device is visible, this module raises.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from .types import (BoxRow, BUF_CDD, BUF_CON, BUF_DIR, BUF_DX0, BUF_KKT, BUF_RIC, BUF_STEP, Dims, Grid,
                    Layout, OPT_BACKWARD_WAVES, OPT_CONDENSE_SPLIT, OPT_CONDENSE_KEEP_QAF, OPT_FXX_STRUCTURE, OPT_GRAPH, OPT_SWITCHING_TRANSPORT, OPT_IMPACT_CONES, OPT_UNCONSTR_DENSE, OPT_LINEARIZE_FUSED, OPT_LINEARIZE_DOFS_PER_PASS, OPT_CONE_JACOBIAN, OPT_MAX_DTS0, OPT_SWEEP_CHUNKS, OPT_WRITEBACK_KKT, OPT_BACKWARD_SCAN, OPT_BACKWARD_REGISTER, OPT_CONDENSE_REGISTER,
                    grid_array)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EXPORTS = [
    "rtoc_version", "rtoc_device_count", "rtoc_dims_supported", "rtoc_create", "rtoc_destroy",
    "rtoc_get_layout", "rtoc_set_grid", "rtoc_set_stream", "rtoc_set_option", "rtoc_upload",
    "rtoc_download", "rtoc_device_ptr", "rtoc_buffer_count", "rtoc_bind", "rtoc_condense",
    "rtoc_riccati_backward", "rtoc_riccati_forward", "rtoc_unconstr_backward",
    "rtoc_unconstr_forward", "rtoc_expand", "rtoc_update", "rtoc_status", "rtoc_clear_status",
    "rtoc_sync", "rtoc_time_phase", "rtoc_set_constraint_rows", "rtoc_gather_directions", "rtoc_error_string",
    "rtoc_riccati_sweep", "rtoc_correct_state_equation", "rtoc_correct_costate_direction",
    "rtoc_compute_initial_state_direction", "rtoc_unconstr_condense", "rtoc_unconstr_expand",
    "rtoc_newton_iteration", "rtoc_converged_count", "rtoc_clone", "rtoc_check_fxx_structure", "rtoc_sto_eval_kkt", "rtoc_set_friction_cones", "rtoc_set_wrench_cones", "rtoc_wrench_cone_matrix", "rtoc_save_stage_dump", "rtoc_load_stage_dump", "rtoc_kkt_error", "rtoc_integrate_solution",
    "rtoc_set_robot_model", "rtoc_robot_model_plan", "rtoc_set_contact_schedule", "rtoc_linearize_contact_dynamics",
    "rtoc_line_search_filter", "rtoc_line_search_clear", "rtoc_set_configuration_cost", "rtoc_set_initial_state",
    "rtoc_unconstr_eval_kkt", "rtoc_unconstr_update_solution", "rtoc_set_constraint_bounds", "rtoc_unconstr_init_constraints", "rtoc_linearize_state_equation", "rtoc_contact_eval_kkt", "rtoc_contact_update_solution",
    "rtoc_set_barrier_param", "rtoc_set_friction_coefficients", "rtoc_contact_init_constraints", "rtoc_set_wrench_cone_params",
    "rtoc_graph_replay_count",
    "rtoc_sto_set_problem", "rtoc_sto_set_regularization", "rtoc_sto_set_cost_terms", "rtoc_sto_init_constraints",
    "rtoc_sto_correct_time_steps", "rtoc_sto_eval_kkt_device", "rtoc_sto_compute_step_sizes", "rtoc_sto_integrate_solution",
    "rtoc_sto_get_event_times", "rtoc_sto_get_time_steps", "rtoc_sto_get_constraint_data", "rtoc_sto_get_kkt_terms",
    "rtoc_sto_set_slack_dual", "rtoc_contact_eval_ocp", "rtoc_set_line_search", "rtoc_contact_line_search",
    "rtoc_bandwidth_probe", "rtoc_get_option",
    "rtoc_set_task_costs", "rtoc_set_grid_times", "rtoc_get_grid_times", "rtoc_set_contact_force_cost",
    "rtoc_set_configuration_ref_table", "rtoc_get_stage_costs",
    "rtoc_parnmpc_set_horizon", "rtoc_parnmpc_init_constraints", "rtoc_parnmpc_init_backward_correction", "rtoc_parnmpc_set_aux_mat",
    "rtoc_parnmpc_get_aux_mat", "rtoc_parnmpc_eval_kkt", "rtoc_parnmpc_backward_correction", "rtoc_parnmpc_update_solution",
    "rtoc_solution_store", "rtoc_solution_interpolate", "rtoc_solution_stored", "rtoc_solution_forget",
    "rtoc_control_policy", "rtoc_control_input",
    "rtoc_set_contact_placements", "rtoc_contact_frame_placements", "rtoc_hold_contact_placements", "rtoc_get_contact_placements",
    "rtoc_set_foot_step_planner", "rtoc_foot_step_planner_init", "rtoc_foot_step_plan", "rtoc_foot_step_plan_get", "rtoc_foot_step_place",
    "rtoc_foot_step_refs", "rtoc_get_task_ref_table", "rtoc_get_configuration_ref_table",
]


LINE_SEARCH_FILTER_CAPACITY = 32  # RTOC_LINE_SEARCH_FILTER_CAPACITY
MAX_PLAN_STEPS = 32  # RTOC_MAX_PLAN_STEPS
FOOT_STEP_FIXED, FOOT_STEP_RAIBERT = 0, 1  # RTOC_FOOT_STEP_*
PROJECT_AS_REFERENCE, PROJECT_YAW = 0, 1  # RTOC_PROJECT_*
GAIT_TROT, GAIT_CRAWL, GAIT_PACE, GAIT_FLYING_TROT = 0, 1, 2, 3  # RTOC_GAIT_*
GAIT_BIPED_WALK = 4  # on two contact surfaces; the others on four point contacts
GAIT_JUMP = 5  # JumpFootStepPlanner: on four point contacts or on two contact surfaces


class FootStepPlanner(C.Structure):
    """include/rtoc_robot.h rtoc_foot_step_planner"""
    _fields_ = [("mode", C.c_int), ("projection", C.c_int), ("enable_stance_phase", C.c_int), ("gait", C.c_int),
                ("swing_time", C.c_double), ("stance_time", C.c_double), ("gain", C.c_double),
                ("step_length", C.c_double * 3), ("step_yaw", C.c_double), ("vcom_cmd", C.c_double * 3), ("yaw_rate_cmd", C.c_double)]


class FootStepRefs(C.Structure):
    """include/rtoc_robot.h rtoc_foot_step_ref_params"""
    _fields_ = [("foot_term", C.c_int * 4), ("com_term", C.c_int), ("configuration", C.c_int),
                ("swing_height", C.c_double * 4), ("swing_start_time", C.c_double * 4), ("period_swing", C.c_double * 4),
                ("period_stance", C.c_double * 4), ("swing_num_phases_in_period", C.c_int * 4),
                ("com_swing_start_time", C.c_double), ("com_period_active", C.c_double), ("com_period_inactive", C.c_double),
                ("com_num_phases_in_period", C.c_int), ("pad0", C.c_int),
                ("q_swing_start_time", C.c_double), ("q_period_active", C.c_double), ("q_period_inactive", C.c_double),
                ("q_num_phases_in_period", C.c_int), ("pad1", C.c_int)]


class RtocError(RuntimeError):
    code = 0   # the RTOC_ERR_* the library returned


ERR_BAD_ARG, ERR_UNSUPPORTED_DIMS, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_READY = -1, -2, -3, -4, -5  # include/rtoc.h


def lib_path():
    # RTOC_HIP_LIB: an alternative build of the same library, e.g. the one with the phase stamps compiled
    # in (make -C robotoc_amd/csrc PROF=1 OUT=../librtoc_hip_prof.so) for tools/phase_profile*.py
    return os.environ.get("RTOC_HIP_LIB") or os.path.join(_HERE, "librtoc_hip.so")


def build(force=False):
    """Compile the HIP kernels + C ABI for gfx950 (hipcc cross-compiles without a GPU): one translation unit per
    robot shape (csrc/Makefile: SHAPES), built in parallel."""
    src_dir = os.path.join(_HERE, "csrc")
    so = lib_path()
    deps = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if os.path.isfile(os.path.join(src_dir, f))]
    deps += [os.path.join(_HERE, "..", "include", f) for f in ("rtoc.h", "rtoc_layout.h")]
    stale = force or not os.path.exists(so) or any(
        os.path.getmtime(d) > os.path.getmtime(so) for d in deps)
    if stale:
        subprocess.check_call(["make", "-C", src_dir, "-j%d" % min(8, os.cpu_count() or 1)] + (["-B"] if force else []),
                              stdout=subprocess.DEVNULL)
    return so


def build_plugin(nv, nu, ns, nw0=None, nw1=None, force=False):
    """Kernel set of one more robot shape as robotoc_amd/librtoc_shape_<nv>_<nu>_<ns>.so (csrc/Makefile: plugin), picked up by
    rtoc_create / rtoc_dims_supported at run time.  Wave counts of the tile-split backward variants default like the library's
    own JIT (RTOC_SHAPE_JIT=1): 1 / 3 up to a 36-wide state, 4 / 4 (5 beyond 64) above."""
    nx = 2 * nv
    nw0 = nw0 if nw0 is not None else (1 if nx <= 36 else 4)
    nw1 = nw1 if nw1 is not None else (3 if nx <= 36 else (5 if nx > 64 else 4))
    so = os.path.join(_HERE, "librtoc_shape_%d_%d_%d.so" % (nv, nu, ns))
    src_dir = os.path.join(_HERE, "csrc")
    deps = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if os.path.isfile(os.path.join(src_dir, f))]
    if force or not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["make", "-C", src_dir, "plugin", "SHAPE=%d:%d:%d:%d:%d" % (nv, nu, ns, nw0, nw1)], stdout=subprocess.DEVNULL)
    return so


def compiled_shapes():
    """(nv, nu, ns) of every robot shape in csrc/Makefile's SHAPES list."""
    import re
    txt = open(os.path.join(_HERE, "csrc", "Makefile")).read()
    m = re.search(r"^SHAPES \?= (.*)$", txt, re.M)
    return [tuple(int(v) for v in tok.split(":")[:3]) for tok in m.group(1).split()]


def lib():
    global _LIB
    if _LIB is None:
        so = lib_path()
        if not os.path.exists(so):
            raise RtocError("librtoc_hip.so not built (run __graft_entry__.build()); "
                            "the HIP path has no CPU fallback")
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        vp = C.c_void_p
        L.rtoc_create.argtypes = [C.POINTER(Dims), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.rtoc_destroy.argtypes = [vp]
        L.rtoc_dims_supported.argtypes = [C.POINTER(Dims)]
        L.rtoc_get_layout.argtypes = [vp, C.POINTER(Layout)]
        L.rtoc_layout_for_dims.argtypes = [C.POINTER(Dims), C.POINTER(Layout)]
        L.rtoc_layout_for_dims.restype = None
        L.rtoc_set_grid.argtypes = [vp, C.POINTER(Grid), C.c_int]
        L.rtoc_set_stream.argtypes = [vp, vp]
        L.rtoc_set_option.argtypes = [vp, C.c_int, C.c_int64]
        L.rtoc_upload.argtypes = [vp, C.c_int, C.c_size_t, dp, C.c_size_t]
        L.rtoc_download.argtypes = [vp, C.c_int, C.c_size_t, dp, C.c_size_t]
        L.rtoc_device_ptr.argtypes = [vp, C.c_int]
        L.rtoc_device_ptr.restype = vp
        L.rtoc_buffer_count.argtypes = [vp, C.c_int]
        L.rtoc_buffer_count.restype = C.c_size_t
        L.rtoc_bind.argtypes = [vp, C.c_int, vp]
        for f in ("rtoc_condense", "rtoc_riccati_backward", "rtoc_riccati_forward", "rtoc_riccati_sweep", "rtoc_update",
                  "rtoc_correct_state_equation", "rtoc_correct_costate_direction",
                  "rtoc_compute_initial_state_direction", "rtoc_unconstr_condense", "rtoc_integrate_solution",
                  "rtoc_linearize_state_equation", "rtoc_contact_eval_kkt", "rtoc_clear_status", "rtoc_sync"):
            getattr(L, f).argtypes = [vp]
        L.rtoc_unconstr_backward.argtypes = [vp, C.c_double]
        L.rtoc_unconstr_forward.argtypes = [vp, C.c_double]
        L.rtoc_unconstr_expand.argtypes = [vp, C.c_double]
        L.rtoc_expand.argtypes = [vp, C.c_double]
        L.rtoc_status.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int]
        L.rtoc_time_phase.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.rtoc_gather_directions.argtypes = [vp, vp, dp]
        L.rtoc_set_constraint_rows.argtypes = [vp, C.POINTER(BoxRow), C.c_int]
        L.rtoc_set_friction_cones.argtypes = [vp, C.c_int, C.c_int]
        L.rtoc_set_wrench_cones.argtypes = [vp, C.c_int]
        L.rtoc_newton_iteration.argtypes = [vp, C.c_double, C.c_double]
        L.rtoc_converged_count.argtypes = [vp, C.POINTER(C.c_int)]
        L.rtoc_wrench_cone_matrix.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
        L.rtoc_save_stage_dump.argtypes = [vp, C.c_char_p, C.c_uint]
        L.rtoc_kkt_error.argtypes = [vp, dp, C.c_int]
        L.rtoc_check_fxx_structure.argtypes = [vp, C.POINTER(C.c_int)]
        L.rtoc_sto_eval_kkt.argtypes = [vp, dp, dp, C.c_int, dp, C.c_int]
        L.rtoc_clone.argtypes = [vp, C.POINTER(vp)]
        L.rtoc_set_robot_model.argtypes = [vp, vp]
        L.rtoc_set_configuration_cost.argtypes = [vp, vp]
        L.rtoc_set_initial_state.argtypes = [vp, dp, C.c_int]
        L.rtoc_unconstr_eval_kkt.argtypes = [vp, C.c_double]
        L.rtoc_set_constraint_bounds.argtypes = [vp, dp, C.c_int, C.c_double, C.c_double]
        L.rtoc_unconstr_init_constraints.argtypes = [vp]
        L.rtoc_contact_init_constraints.argtypes = [vp]
        L.rtoc_set_barrier_param.argtypes = [vp, C.c_double, C.c_double]
        L.rtoc_set_friction_coefficients.argtypes = [vp, dp, C.c_int]
        L.rtoc_set_wrench_cone_params.argtypes = [vp, dp, C.c_int]
        L.rtoc_unconstr_update_solution.argtypes = [vp, C.c_double, dp, C.c_int]
        L.rtoc_contact_update_solution.argtypes = [vp, C.c_double, dp, C.c_int]
        L.rtoc_line_search_filter.argtypes = [vp, dp, dp, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]
        L.rtoc_line_search_clear.argtypes = [vp]
        L.rtoc_linearize_contact_dynamics.argtypes = [vp, C.c_int]
        L.rtoc_set_contact_schedule.argtypes = [vp, C.POINTER(C.c_uint), dp, dp]
        L.rtoc_load_stage_dump.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
        L.rtoc_graph_replay_count.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.rtoc_sto_set_problem.argtypes = [vp, C.c_double, C.c_double, dp, C.c_int, C.c_int, dp, C.c_double, C.c_double]
        L.rtoc_sto_set_regularization.argtypes = [vp, C.c_double]
        L.rtoc_sto_set_cost_terms.argtypes = [vp, dp, dp]
        for f in ("rtoc_sto_init_constraints", "rtoc_sto_correct_time_steps", "rtoc_sto_eval_kkt_device",
                  "rtoc_sto_compute_step_sizes", "rtoc_sto_integrate_solution"):
            getattr(L, f).argtypes = [vp]
        for f in ("rtoc_sto_get_event_times", "rtoc_sto_get_time_steps", "rtoc_sto_get_constraint_data"):
            getattr(L, f).argtypes = [vp, dp, C.c_int]
        L.rtoc_sto_get_kkt_terms.argtypes = [vp, dp, dp, dp, C.c_int]
        L.rtoc_sto_set_slack_dual.argtypes = [vp, dp, dp]
        L.rtoc_contact_eval_ocp.argtypes = [vp, C.c_int, dp, dp, C.c_int]
        L.rtoc_set_line_search.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
        L.rtoc_contact_line_search.argtypes = [vp, C.POINTER(C.c_int)]
        L.rtoc_error_string.argtypes = [C.c_int]
        L.rtoc_error_string.restype = C.c_char_p
        L.rtoc_set_task_costs.argtypes = [vp, vp, C.c_int, C.c_int]
        L.rtoc_set_grid_times.argtypes = [vp, dp, C.c_int]
        L.rtoc_set_task_ref_table.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
        L.rtoc_get_grid_times.argtypes = [vp, dp, C.c_int]
        L.rtoc_set_contact_force_cost.argtypes = [vp, vp, C.c_int]
        L.rtoc_get_stage_costs.argtypes = [vp, dp, C.c_int]
        L.rtoc_set_configuration_ref_table.argtypes = [vp, dp, C.POINTER(C.c_int), C.c_int, C.c_int]
        L.rtoc_parnmpc_set_horizon.argtypes = [vp, C.c_int]
        L.rtoc_parnmpc_init_constraints.argtypes = [vp]
        L.rtoc_parnmpc_init_backward_correction.argtypes = [vp]
        L.rtoc_parnmpc_set_aux_mat.argtypes = [vp, dp, C.c_int]
        L.rtoc_parnmpc_get_aux_mat.argtypes = [vp, dp, C.c_int]
        L.rtoc_parnmpc_eval_kkt.argtypes = [vp, C.c_double]
        L.rtoc_parnmpc_backward_correction.argtypes = [vp, C.c_double]
        L.rtoc_parnmpc_update_solution.argtypes = [vp, C.c_double, dp, C.c_int]
        L.rtoc_solution_store.argtypes = [vp, C.c_double]
        L.rtoc_solution_interpolate.argtypes = [vp, C.c_double]
        L.rtoc_solution_stored.argtypes = [vp, C.POINTER(C.c_int)]
        L.rtoc_solution_forget.argtypes = [vp]
        L.rtoc_control_policy.argtypes = [vp, C.c_double, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int]
        L.rtoc_control_input.argtypes = [vp, C.c_double, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int]
        L.rtoc_set_contact_placements.argtypes = [vp, dp, dp, C.c_int]
        L.rtoc_contact_frame_placements.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, C.c_int]
        L.rtoc_hold_contact_placements.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
        L.rtoc_get_contact_placements.argtypes = [vp, dp, dp, C.c_int, C.POINTER(C.c_int)]
        ip = C.POINTER(C.c_int)
        L.rtoc_set_foot_step_planner.argtypes = [vp, vp, C.c_int]
        L.rtoc_foot_step_planner_init.argtypes = [vp]
        L.rtoc_foot_step_plan.argtypes = [vp, C.c_double, C.c_uint, C.c_int]
        L.rtoc_foot_step_plan_get.argtypes = [vp, dp, dp, dp, dp, ip, C.c_int, ip, ip]
        L.rtoc_foot_step_place.argtypes = [vp, ip, C.c_int]
        L.rtoc_foot_step_refs.argtypes = [vp, vp, ip, C.POINTER(C.c_uint), C.c_int, C.c_int]
        L.rtoc_get_task_ref_table.argtypes = [vp, C.c_int, vp, C.c_int, ip]
        L.rtoc_get_configuration_ref_table.argtypes = [vp, dp, ip, C.c_int, ip]
        _LIB = L
    return _LIB


def layout_for(dims):
    out = Layout()
    lib().rtoc_layout_for_dims(C.byref(dims), C.byref(out))
    return out


def _chk(rc):
    if rc != 0:
        e = RtocError("rtoc error %d: %s" % (rc, lib().rtoc_error_string(rc).decode()))
        e.code = rc
        raise e


def _dp(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Context:
    """Thin RAII wrapper over rtoc_ctx: one context per (device, problem shape, batch)."""
    _fs_gait = GAIT_TROT   # the gait of the foot-step planner in force and the contacts of the model it was set for: the feet decide
    _fs_ncontacts = 4      # the layout of rtoc_foot_step_plan_get's positions

    def __init__(self, dims, max_stages, batch, device=0):
        self.dims = dims
        self.batch = batch
        self.max_stages = max_stages
        self._h = C.c_void_p()
        _chk(lib().rtoc_create(C.byref(dims), max_stages, batch, device, C.byref(self._h)))
        self.L = Layout()
        _chk(lib().rtoc_get_layout(self._h, C.byref(self.L)))
        self.nstages = 0

    @classmethod
    def from_stage_dump(cls, path, device=0):
        """rtoc_load_stage_dump: a context restored from a stage dump (robotoc_amd/replay.py format)."""
        from .replay import read_dump
        meta = read_dump(path)
        self = cls.__new__(cls)
        self.dims = meta["dims"]
        self.batch = meta["batch"]
        self.max_stages = len(meta["grids"])
        self._h = C.c_void_p()
        _chk(lib().rtoc_load_stage_dump(str(path).encode(), device, C.byref(self._h)))
        self.L = Layout()
        _chk(lib().rtoc_get_layout(self._h, C.byref(self.L)))
        self.nstages = len(meta["grids"])
        return self

    def close(self):
        if self._h:
            lib().rtoc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_grid(self, grids):
        g = grid_array(grids)
        _chk(lib().rtoc_set_grid(self._h, g, len(grids)))
        self.nstages = len(grids)

    def set_constraint_rows(self, rows):
        arr = (BoxRow * max(len(rows), 1))()
        for i, r in enumerate(rows):
            arr[i] = r
        _chk(lib().rtoc_set_constraint_rows(self._h, arr, len(rows)))

    def set_stream(self, hip_stream):
        _chk(lib().rtoc_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_writeback(self, on):
        _chk(lib().rtoc_set_option(self._h, OPT_WRITEBACK_KKT, int(bool(on))))

    def set_max_dts0(self, v):
        bits = struct.unpack("<q", struct.pack("<d", float(v)))[0]
        _chk(lib().rtoc_set_option(self._h, OPT_MAX_DTS0, bits))

    def set_contact_inv_damping(self, v):
        bits = struct.unpack("<q", struct.pack("<d", float(v)))[0]
        _chk(lib().rtoc_set_option(self._h, 3, bits))

    def set_backward_waves(self, nw):
        _chk(lib().rtoc_set_option(self._h, OPT_BACKWARD_WAVES, int(nw)))

    def upload(self, buffer, arr, offset=0):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        _chk(lib().rtoc_upload(self._h, buffer, offset, _dp(arr), arr.size))

    def download(self, buffer, shape, offset=0):
        out = np.empty(shape, dtype=np.float64)
        _chk(lib().rtoc_download(self._h, buffer, offset, _dp(out), out.size))
        return out

    def device_ptr(self, buffer):
        return lib().rtoc_device_ptr(self._h, buffer)

    def buffer_count(self, buffer):
        return lib().rtoc_buffer_count(self._h, buffer)

    def bind(self, buffer, device_ptr):
        _chk(lib().rtoc_bind(self._h, buffer, C.c_void_p(device_ptr)))

    def condense(self):
        _chk(lib().rtoc_condense(self._h))

    def riccati_backward(self):
        _chk(lib().rtoc_riccati_backward(self._h))

    def riccati_forward(self):
        _chk(lib().rtoc_riccati_forward(self._h))

    def riccati_sweep(self):
        """backward + forward, pipelined over instance chunks (rtoc_riccati_sweep)."""
        _chk(lib().rtoc_riccati_sweep(self._h))

    def set_sweep_chunks(self, n):
        _chk(lib().rtoc_set_option(self._h, OPT_SWEEP_CHUNKS, int(n)))

    def newton_iteration(self, kkt_tol, tau=0.995):
        """rtoc_newton_iteration: KKT error -> condense -> sweep -> expand -> converged-instance mask ->
        update -> integrate, one launch sequence; returns nothing (asynchronous)."""
        _chk(lib().rtoc_newton_iteration(self._h, float(kkt_tol), float(tau)))

    def converged_count(self):
        n = C.c_int(0)
        _chk(lib().rtoc_converged_count(self._h, C.byref(n)))
        return n.value

    def set_backward_scan(self, on):
        """RTOC_OPT_BACKWARD_SCAN: backward recursion as a scan over the horizon (few instances, low latency)."""
        _chk(lib().rtoc_set_option(self._h, OPT_BACKWARD_SCAN, 2 if on == "auto" else int(bool(on))))

    def set_condense_register(self, on=True):
        """RTOC_OPT_CONDENSE_REGISTER: the register-chained condensation kernel (one wave per contact grid point) where it applies;
        "cones": also in contexts with friction / wrench cone rows."""
        _chk(lib().rtoc_set_option(self._h, OPT_CONDENSE_REGISTER, 2 if on == "cones" else int(bool(on))))

    def set_backward_register(self, on):
        """RTOC_OPT_BACKWARD_REGISTER: the register-resident backward kernel (one wave per instance) where it applies;
        2: the iCub-size shapes' register-wide kernel on every batch size (1: on batches larger than the device's CU count)."""
        _chk(lib().rtoc_set_option(self._h, OPT_BACKWARD_REGISTER, 2 if on == 2 else int(bool(on))))

    def set_condense_split(self, on):
        """RTOC_OPT_CONDENSE_SPLIT: MJtJinv in its own kernel or one fused condensation kernel (default per robot shape)."""
        _chk(lib().rtoc_set_option(self._h, OPT_CONDENSE_SPLIT, int(bool(on))))

    def get_option(self, option):
        """rtoc_get_option: the value in force of an integer-valued option"""
        v = C.c_int64(0)
        lib().rtoc_get_option.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        _chk(lib().rtoc_get_option(self._h, int(option), C.byref(v)))
        return int(v.value)

    def set_condense_keep_qaf(self, on):
        """RTOC_OPT_CONDENSE_KEEP_QAF: also store Qafqv / Qafu_full in the ContactDynamicsData record."""
        _chk(lib().rtoc_set_option(self._h, OPT_CONDENSE_KEEP_QAF, int(bool(on))))

    def sto_eval_kkt(self, lt, qtt_diag):
        """rtoc_sto_eval_kkt: lt, qtt_diag [batch, num_events]; returns the squared STO KKT-error term per instance."""
        lt = np.ascontiguousarray(lt, dtype=np.float64)
        qtt_diag = np.ascontiguousarray(qtt_diag, dtype=np.float64)
        assert lt.shape == qtt_diag.shape and lt.shape[0] == self.batch
        out = np.zeros(self.batch)
        _chk(lib().rtoc_sto_eval_kkt(self._h, _dp(lt), _dp(qtt_diag), lt.shape[1], _dp(out), self.batch))
        return out

    # ---- SwitchingTimeOptimization resident on the device (rtoc.h: rtoc_sto_*) ----
    STO_MAX_ROWS = 16

    def sto_set_problem(self, t0, T, event_times, min_dwell_times, barrier_param=1.0e-3, fraction_to_boundary_rule=0.995):
        """event_times: [num_events] (shared by the batch) or [batch, num_events]; min_dwell_times: [num_events + 1]."""
        et = np.ascontiguousarray(event_times, dtype=np.float64)
        md = np.ascontiguousarray(min_dwell_times, dtype=np.float64)
        nev = et.shape[-1] if et.size else 0
        assert et.ndim in (1, 2) and (et.ndim == 1 or et.shape[0] == self.batch) and md.size == nev + 1
        _chk(lib().rtoc_sto_set_problem(self._h, t0, T, _dp(et), nev, int(et.ndim == 2), _dp(md), barrier_param, fraction_to_boundary_rule))
        self.sto_nev = nev

    def sto_set_regularization(self, sto_reg):
        _chk(lib().rtoc_sto_set_regularization(self._h, sto_reg))

    def sto_set_cost_terms(self, lt=None, qtt_diag=None):
        if lt is None:
            _chk(lib().rtoc_sto_set_cost_terms(self._h, None, None))
            return
        lt, qtt_diag = np.ascontiguousarray(lt, dtype=np.float64), np.ascontiguousarray(qtt_diag, dtype=np.float64)
        assert lt.shape == qtt_diag.shape == (self.batch, self.sto_nev)
        _chk(lib().rtoc_sto_set_cost_terms(self._h, _dp(lt), _dp(qtt_diag)))

    def sto_init_constraints(self):
        _chk(lib().rtoc_sto_init_constraints(self._h))

    def sto_set_slack_dual(self, slack, dual):
        slack, dual = np.ascontiguousarray(slack, dtype=np.float64), np.ascontiguousarray(dual, dtype=np.float64)
        assert slack.shape == dual.shape == (self.batch, self.sto_nev + 1)
        _chk(lib().rtoc_sto_set_slack_dual(self._h, _dp(slack), _dp(dual)))

    def sto_correct_time_steps(self):
        _chk(lib().rtoc_sto_correct_time_steps(self._h))

    def sto_eval_kkt_device(self):
        _chk(lib().rtoc_sto_eval_kkt_device(self._h))

    def sto_compute_step_sizes(self):
        _chk(lib().rtoc_sto_compute_step_sizes(self._h))

    def sto_integrate_solution(self):
        _chk(lib().rtoc_sto_integrate_solution(self._h))

    def sto_event_times(self):
        out = np.zeros((self.batch, self.sto_nev))
        _chk(lib().rtoc_sto_get_event_times(self._h, _dp(out), self.batch))
        return out

    def sto_time_steps(self):
        out = np.zeros((self.batch, self.nstages))
        _chk(lib().rtoc_sto_get_time_steps(self._h, _dp(out), self.batch))
        return out

    def sto_constraint_data(self):
        """[batch, 6, num_events + 1]: slack, dual, residual, cmpl, dslack, ddual of the dwell-time rows."""
        out = np.zeros((self.batch, 6, self.STO_MAX_ROWS))
        _chk(lib().rtoc_sto_get_constraint_data(self._h, _dp(out), self.batch))
        return out[:, :, :self.sto_nev + 1].copy()

    def sto_kkt_terms(self):
        """(lt, diag Qtt, squared STO KKT term) of the last SwitchingTimeOptimization::evalKKT on the device."""
        lt, qtt, err = np.zeros((self.batch, self.sto_nev)), np.zeros((self.batch, self.sto_nev)), np.zeros(self.batch)
        _chk(lib().rtoc_sto_get_kkt_terms(self._h, _dp(lt), _dp(qtt), _dp(err), self.batch))
        return lt, qtt, err

    def graph_replay_count(self):
        n = C.c_ulonglong()
        _chk(lib().rtoc_graph_replay_count(self._h, C.byref(n)))
        return int(n.value)

    def set_graph(self, on):
        """RTOC_OPT_GRAPH: replay rtoc_riccati_sweep / rtoc_newton_iteration from captured hipGraphs."""
        _chk(lib().rtoc_set_option(self._h, OPT_GRAPH, int(bool(on))))

    def set_switching_transport(self, exact):
        """RTOC_OPT_SWITCHING_TRANSPORT: free-flyer block of the switching-constraint Jacobians -- False (default): as the
        reference composes it (Pq dIntegrate^T); True: the chain rule (Pq dIntegrate)."""
        _chk(lib().rtoc_set_option(self._h, OPT_SWITCHING_TRANSPORT, int(bool(exact))))

    def set_fxx_structure(self, mode):
        """RTOC_OPT_FXX_STRUCTURE: 0 automatic (checked on the device), 1 always dense, 2 caller asserts the structure."""
        _chk(lib().rtoc_set_option(self._h, OPT_FXX_STRUCTURE, int(mode)))

    def check_fxx_structure(self):
        """rtoc_check_fxx_structure: True iff every resident Fxx has the state-equation structure."""
        out = C.c_int(0)
        _chk(lib().rtoc_check_fxx_structure(self._h, C.byref(out)))
        return bool(out.value)

    def correct_state_equation(self):
        _chk(lib().rtoc_correct_state_equation(self._h))

    def correct_costate_direction(self):
        _chk(lib().rtoc_correct_costate_direction(self._h))

    def compute_initial_state_direction(self):
        _chk(lib().rtoc_compute_initial_state_direction(self._h))

    def integrate_solution(self):
        _chk(lib().rtoc_integrate_solution(self._h))

    # ---- filter line search (line_search_filter.cpp), batched ----
    def line_search_filter(self, cost, violation, mask=None, cost_reduction_rate=0.005, constraint_violation_reduction_rate=0.005):
        """rtoc_line_search_filter: accept test + filter update of every instance; returns accepted [batch] (0/1).
        Default rates: LineSearchSettings (include/robotoc/line_search/line_search_settings.hpp)."""
        cost = np.ascontiguousarray(cost, dtype=np.float64)
        violation = np.ascontiguousarray(violation, dtype=np.float64)
        n = cost.shape[0]
        acc = np.zeros(n, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        _chk(lib().rtoc_line_search_filter(self._h, _dp(cost), _dp(violation), m.ctypes.data_as(ip) if m is not None else None, n,
                                           cost_reduction_rate, constraint_violation_reduction_rate, acc.ctypes.data_as(ip)))
        return acc

    def contact_eval_ocp(self, trial=False):
        """rtoc_contact_eval_ocp: (cost + cost_barrier, primal_feasibility) of every instance"""
        cost, viol = np.zeros(self.batch), np.zeros(self.batch)
        _chk(lib().rtoc_contact_eval_ocp(self._h, int(bool(trial)), _dp(cost), _dp(viol), self.batch))
        return cost, viol

    def set_line_search(self, enable=True, step_size_reduction_rate=0.75, min_step_size=0.05, filter_cost_reduction_rate=0.005,
                        filter_constraint_violation_reduction_rate=0.005):
        """SolverOptions::enable_line_search + LineSearchSettings (filter method)"""
        _chk(lib().rtoc_set_line_search(self._h, int(bool(enable)), step_size_reduction_rate, min_step_size, filter_cost_reduction_rate,
                                        filter_constraint_violation_reduction_rate))

    def set_line_search_method(self, method="filter", armijo_control_rate=0.001, margin_rate=0.05, eps=1.0e-8):
        """LineSearchSettings::line_search_method: "filter" (default) or "merit" (LineSearch::meritBacktrackingLineSearch)"""
        lib().rtoc_set_line_search_method.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
        _chk(lib().rtoc_set_line_search_method(self._h, {"filter": 0, "merit": 1}[method], armijo_control_rate, margin_rate, eps))

    def line_search_trials(self):
        n = C.c_int()
        _chk(lib().rtoc_line_search_trials(self._h, C.byref(n)))
        return n.value

    def line_search_merit_terms(self):
        p, d = np.zeros(self.batch), np.zeros(self.batch)
        lib().rtoc_line_search_merit_terms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        _chk(lib().rtoc_line_search_merit_terms(self._h, _dp(p), _dp(d), self.batch))
        return p, d

    def contact_line_search(self):
        n = C.c_int()
        _chk(lib().rtoc_contact_line_search(self._h, C.byref(n)))
        return n.value

    def line_search_clear(self):
        _chk(lib().rtoc_line_search_clear(self._h))

    # ---- SolutionInterpolator on the device (include/rtoc_robot.h: rtoc_solution_*) ----
    def solution_store(self, t0):
        """rtoc_solution_store: snapshot RTOC_BUF_SOL with the grid, the contact schedule and the grid times summed from t0 (with an
        STO problem every instance's own: sto_correct_time_steps first)"""
        _chk(lib().rtoc_solution_store(self._h, float(t0)))

    def solution_interpolate(self, t0):
        """rtoc_solution_interpolate: every record of RTOC_BUF_SOL for the current grid, schedule and time steps (times from t0) from
        the stored solution; nothing happens with nothing stored"""
        _chk(lib().rtoc_solution_interpolate(self._h, float(t0)))

    def solution_stored(self):
        """rtoc_solution_stored: the grid points of the stored solution, 0 if there is none"""
        n = C.c_int(0)
        _chk(lib().rtoc_solution_stored(self._h, C.byref(n)))
        return n.value

    def solution_forget(self):
        _chk(lib().rtoc_solution_forget(self._h))

    # ---- ControlPolicy on the device (include/rtoc_robot.h: rtoc_control_policy / rtoc_control_input) ----
    def _policy_times(self, t, count):
        """(t as a contiguous array, per_instance, count): a scalar is shared by the batch, else one time per instance"""
        t = np.asarray(t, dtype=np.float64)   # (ascontiguousarray would turn a scalar into one time per instance of a batch of 1)
        if t.ndim == 0:
            return t.reshape(1), 0, self.batch if count is None else int(count)
        if t.ndim != 1 or (count is not None and t.size != count):
            raise ValueError("t must be a scalar or one time per instance, not %s" % (t.shape,))
        return np.ascontiguousarray(t), 1, t.size

    def control_policy(self, t0, t, N, count=None):
        """rtoc_control_policy: the policy of the first `count` instances (default: all with a scalar `t`, else len(t)) at time `t`
        (a scalar shared by the batch, or one time per instance) over the grid times summed from t0, N = the number of time stages.
        Returns {"tauJ", "qJ", "dqJ": [count, nu], "Kp", "Kd": [count, nu, nu]}."""
        from .types import control_policy_offsets
        t, per_instance, count = self._policy_times(t, count)
        nu = self.dims.nu
        off, stride = control_policy_offsets(nu)
        out = np.empty((count, stride))
        _chk(lib().rtoc_control_policy(self._h, float(t0), t.ctypes.data, per_instance, int(N), out.ctypes.data, count, 0))
        res = {k: out[:, off[k]:off[k] + nu].copy() for k in ("tauJ", "qJ", "dqJ")}
        for k in ("Kp", "Kd"):   # column-major, leading dimension nu
            res[k] = np.ascontiguousarray(out[:, off[k]:off[k] + nu * nu].reshape(count, nu, nu).swapaxes(1, 2))
        return res

    def control_input(self, t0, t, N, x):
        """rtoc_control_input: u [count, nu] = tauJ - Kp (qJ - q) - Kd (dqJ - v) of the policy at `t` (as for control_policy) at the
        measured states x [count, nq + nv] (laid out as for set_initial_state)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nx = 2 * self.dims.nv + (1 if self.dims.np == 6 else 0)
        if x.ndim != 2 or x.shape[1] != nx:
            raise ValueError("x must be [count, %d], not %s" % (nx, x.shape))
        t, per_instance, count = self._policy_times(t, x.shape[0])
        u = np.empty((count, self.dims.nu))
        _chk(lib().rtoc_control_input(self._h, float(t0), t.ctypes.data, per_instance, int(N), x.ctypes.data, u.ctypes.data, count, 0))
        return u

    # ---- rigid-body linearisation (include/rtoc_robot.h) ----
    def set_robot_model(self, model):
        """rtoc_set_robot_model: `model` = robotoc_amd.robot_model.RobotModel"""
        _chk(lib().rtoc_set_robot_model(self._h, C.byref(model)))
        self._model_ncontacts = model.ncontacts

    def set_contact_schedule(self, active, positions=None, rotations=None):
        """rtoc_set_contact_schedule: active [nstages] bit masks, positions [nstages, ncontacts, 3] or None,
        rotations [nstages, ncontacts, 3, 3] (row-major; surface contacts) or None"""
        act = np.ascontiguousarray(active, dtype=np.uint32)
        assert act.shape == (self.nstages,)
        pos = rot = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.float64)
            assert pos.shape == (self.nstages, self._model_ncontacts, 3)
        if rotations is not None:
            rot = np.ascontiguousarray(rotations, dtype=np.float64).reshape(self.nstages, self._model_ncontacts, 9)
        _chk(lib().rtoc_set_contact_schedule(self._h, act.ctypes.data_as(C.POINTER(C.c_uint)), _dp(pos) if pos is not None else None,
                                             _dp(rot) if rot is not None else None))

    def set_contact_placements(self, positions, rotations=None):
        """rtoc_set_contact_placements: the placements of the schedule in force, its masks kept -- positions [nstages, ncontacts, 3]
        shared by the batch or [batch, nstages, ncontacts, 3] (every instance its own footholds: the leading dimension decides) or
        None (zeros), rotations with the same leading shape and [..., 3, 3] or [..., 9] (row-major) or None (identity)"""
        n, nc = self.nstages, self._model_ncontacts
        pos = rot = None
        lead = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.float64)
            if pos.shape not in ((n, nc, 3), (self.batch, n, nc, 3)):
                raise ValueError("positions must be [%d, %d, 3] or [%d, %d, %d, 3], not %s" % (n, nc, self.batch, n, nc, pos.shape))
            lead = pos.shape[:-3]
        if rotations is not None:
            rot = np.ascontiguousarray(rotations, dtype=np.float64)
            if rot.shape[-2:] == (3, 3):
                rot = rot.reshape(rot.shape[:-2] + (9,))
            if rot.shape not in ((n, nc, 9), (self.batch, n, nc, 9)):
                raise ValueError("rotations must be [%d, %d, 3, 3] or [%d, %d, %d, 3, 3], not %s" % (n, nc, self.batch, n, nc, rot.shape))
            if lead is not None and rot.shape[:-3] != lead:
                raise ValueError("positions and rotations must both be shared or both per instance")
            lead = rot.shape[:-3]
        _chk(lib().rtoc_set_contact_placements(self._h, _dp(pos) if pos is not None else None, _dp(rot) if rot is not None else None,
                                               1 if lead else 0))

    def contact_placements(self):
        """rtoc_get_contact_placements: (positions [batch, nstages, ncontacts, 3], rotations [batch, nstages, ncontacts, 3, 3],
        per_instance) -- the table as the instances read it (a shared one repeated; zeros / identities where none was set)"""
        n, nc = self.nstages, self._model_ncontacts
        pos, rot, inst = np.zeros((self.batch, n, nc, 3)), np.zeros((self.batch, n, nc, 9)), C.c_int(0)
        _chk(lib().rtoc_get_contact_placements(self._h, _dp(pos), _dp(rot), self.batch, C.byref(inst)))
        return pos, rot.reshape(self.batch, n, nc, 3, 3), bool(inst.value)

    _PLACEMENT_SOURCES = {"x0": 0, "sol": 1}

    def contact_frame_placements(self, source="x0", grid_point=0):
        """rtoc_contact_frame_placements: (R [batch, ncontacts, 3, 3], p [batch, ncontacts, 3], com [batch, 3]) -- world rotation
        and position of every contact frame and the centre of mass of every instance, at the q of set_initial_state (source "x0")
        or at q of grid point `grid_point` of BUF_SOL (source "sol")"""
        nc = self._model_ncontacts
        R, p, com = np.zeros((self.batch, nc, 9)), np.zeros((self.batch, nc, 3)), np.zeros((self.batch, 3))
        _chk(lib().rtoc_contact_frame_placements(self._h, self._PLACEMENT_SOURCES[source], int(grid_point), _dp(R), _dp(p), _dp(com), self.batch))
        return R.reshape(self.batch, nc, 3, 3), p, com

    def hold_contact_placements(self, contacts, first=0, last=None, source="x0", grid_point=0):
        """rtoc_hold_contact_placements: on the device, write where the contact frames in the bit mask `contacts` are now (at the q
        of `source`, as for contact_frame_placements) into grid points [first, last) of every instance's own placement table (last =
        None: to the end of the grid).  A shared table becomes per instance, every instance starting from the shared values."""
        _chk(lib().rtoc_hold_contact_placements(self._h, self._PLACEMENT_SOURCES[source], int(grid_point), int(first),
                                                self.nstages if last is None else int(last), int(contacts)))

    def clone(self):
        """rtoc_clone: a second context with the same configuration, state and records"""
        h = C.c_void_p()
        _chk(lib().rtoc_clone(self._h, C.byref(h)))
        twin = Context.__new__(Context)
        twin.__dict__.update(self.__dict__)
        twin._h = h
        return twin

    # ---- TrotFootStepPlanner and the MPC references on the device (include/rtoc_robot.h) ----
    def set_foot_step_planner(self, planner):
        """rtoc_set_foot_step_planner: `planner` = a FootStepPlanner struct for the batch, a list of `batch` of them (every instance its
        own command), or None (removes the planner)"""
        if planner is None:
            _chk(lib().rtoc_set_foot_step_planner(self._h, None, 0))
            return
        per_instance = not isinstance(planner, FootStepPlanner)
        rows = list(planner) if per_instance else [planner]
        if per_instance and len(rows) != self.batch:
            raise ValueError("per-instance commands need one planner struct per instance")
        arr = (FootStepPlanner * len(rows))(*rows)
        _chk(lib().rtoc_set_foot_step_planner(self._h, C.cast(arr, C.c_void_p), 1 if per_instance else 0))
        self._fs_gait = rows[0].gait   # (a refused call raised above and leaves the planner in force)
        self._fs_ncontacts = self._model_ncontacts

    def foot_step_planner_init(self):
        """rtoc_foot_step_planner_init: the planner's init (one for the four quadruped gaits, the biped walk's own) at the q of set_initial_state, every instance"""
        _chk(lib().rtoc_foot_step_planner_init(self._h))

    def foot_step_plan(self, t, contact_status0, planning_steps):
        """rtoc_foot_step_plan: plan() of the planner's gait (FootStepPlanner.gait, GAIT_*) from the q, v of set_initial_state;
        contact_status0 = the bit mask of the contacts active in the first phase"""
        _chk(lib().rtoc_foot_step_plan(self._h, float(t), int(contact_status0), int(planning_steps)))

    def foot_step_plan_get(self):
        """rtoc_foot_step_plan_get: a dict -- positions [batch, size, 4, 3], com [batch, size, 3], R [batch, size, 3, 3],
        step_length [batch, 3], ok [batch] (bool), size, current_step.  A planner on two feet (gait = GAIT_BIPED_WALK was set last, or
        GAIT_JUMP on a model of two contact surfaces): positions [batch, size, 2, 3] and one more key, surfaces [batch, size, 2, 3, 3]"""
        B, S = self.batch, MAX_PLAN_STEPS + 2
        two = self._fs_gait == GAIT_BIPED_WALK or (self._fs_gait == GAIT_JUMP and self._fs_ncontacts == 2)
        w = 24 if two else 12   # the library's `positions` per (instance, step): [4][3], or [2][3] and [2][9] behind them
        pos, com, R, sl = np.zeros((B, S * w)), np.zeros((B, S * 3)), np.zeros((B, S * 9)), np.zeros((B, 3))
        ok, size, cur = np.zeros(B, dtype=np.int32), C.c_int(0), C.c_int(0)
        _chk(lib().rtoc_foot_step_plan_get(self._h, _dp(pos), _dp(com), _dp(R), _dp(sl), ok.ctypes.data_as(C.POINTER(C.c_int)), B,
                                           C.byref(size), C.byref(cur)))
        n = size.value   # the library packs [count][size][...] densely at the front of the arrays
        out = dict(com=com.reshape(-1)[:B * n * 3].reshape(B, n, 3).copy(),
                   R=R.reshape(-1)[:B * n * 9].reshape(B, n, 3, 3).copy(), step_length=sl, ok=ok != 0, size=n, current_step=cur.value)
        pos = pos.reshape(-1)[:B * n * w].reshape(B, n, w)
        if two:
            out["positions"], out["surfaces"] = pos[:, :, :6].reshape(B, n, 2, 3).copy(), pos[:, :, 6:].reshape(B, n, 2, 3, 3).copy()
        else:
            out["positions"] = pos.reshape(B, n, 4, 3).copy()
        return out

    def foot_step_place(self, phase_of_grid_point):
        """rtoc_foot_step_place: grid point i of every instance <- contactPositions(phase_of_grid_point[i] + 1) of its plan (the
        biped walk: contactPlacements, the rotations into the per-instance rotation table)"""
        ph = np.ascontiguousarray(phase_of_grid_point, dtype=np.int32)
        _chk(lib().rtoc_foot_step_place(self._h, ph.ctypes.data_as(C.POINTER(C.c_int)), ph.size))

    def foot_step_refs(self, refs, phase_of_grid_point=None, phase_masks=None):
        """rtoc_foot_step_refs: `refs` = a FootStepRefs struct; the swing-foot, CoM and configuration references of every
        (instance, grid point) into the per-instance reference tables.  The jump (GAIT_JUMP) writes its one configuration reference on
        every row of the grid in force and reads no phases: both may be None, which passes NULL"""
        if phase_of_grid_point is None:
            ph_p, nstages = None, self.nstages
        else:
            ph = np.ascontiguousarray(phase_of_grid_point, dtype=np.int32)
            ph_p, nstages = ph.ctypes.data_as(C.POINTER(C.c_int)), ph.size
        if phase_masks is None:
            mk_p, nphases = None, 0
        else:
            mk = np.ascontiguousarray(phase_masks, dtype=np.uint32)
            mk_p, nphases = mk.ctypes.data_as(C.POINTER(C.c_uint)), mk.size
        _chk(lib().rtoc_foot_step_refs(self._h, C.cast(C.pointer(refs), C.c_void_p), ph_p, mk_p, nphases, nstages))

    def task_ref_table(self, term):
        """rtoc_get_task_ref_table: (R [batch, nstages, 3, 3], p [batch, nstages, 3], active [batch, nstages] (bool), per_instance)
        -- the table of term `term` as the instances read it"""
        raw = np.zeros((self.batch, self.nstages, 13))
        inst = C.c_int(0)
        _chk(lib().rtoc_get_task_ref_table(self._h, int(term), raw.ctypes.data_as(C.c_void_p), self.batch, C.byref(inst)))
        flags = np.ascontiguousarray(raw[..., 12]).view(np.int32).reshape(self.batch, self.nstages, 2)
        return raw[..., :9].reshape(self.batch, self.nstages, 3, 3).copy(), raw[..., 9:12].copy(), flags[..., 0] != 0, bool(inst.value)

    def configuration_ref_table(self):
        """rtoc_get_configuration_ref_table: (q_ref [batch, nstages, nq], active [batch, nstages] (bool), per_instance)"""
        nq = self.dims.nv + (1 if self.dims.np == 6 else 0)
        q, act, inst = np.zeros((self.batch, self.nstages, nq)), np.zeros((self.batch, self.nstages), dtype=np.int32), C.c_int(0)
        _chk(lib().rtoc_get_configuration_ref_table(self._h, _dp(q), act.ctypes.data_as(C.POINTER(C.c_int)), self.batch, C.byref(inst)))
        return q, act != 0, bool(inst.value)

    def set_configuration_cost(self, q_ref, v_ref, u_ref, q_weight, v_weight, a_weight, u_weight, q_weight_terminal, v_weight_terminal,
                               q_weight_impact=None, v_weight_impact=None, dv_weight_impact=None):
        """rtoc_set_configuration_cost (ConfigurationSpaceCost; q_ref on the manifold: nq entries)"""
        from .robot_model import MAX_JOINTS
        arr = np.zeros((12, MAX_JOINTS))
        z = np.zeros(self.dims.nv)
        vals = (q_ref, v_ref, u_ref, q_weight, v_weight, a_weight, u_weight, q_weight_terminal, v_weight_terminal,
                z if q_weight_impact is None else q_weight_impact, z if v_weight_impact is None else v_weight_impact,
                z if dv_weight_impact is None else dv_weight_impact)
        for k, v in enumerate(vals):
            v = np.asarray(v, dtype=np.float64)
            arr[k, :v.size] = v
        _chk(lib().rtoc_set_configuration_cost(self._h, arr.ctypes.data_as(C.c_void_p)))

    def set_configuration_ref_table(self, q_ref, active=None):
        """rtoc_set_configuration_ref_table: a time-varying q_ref (ConfigurationSpaceRefBase) -- `q_ref` [nstages, nq] shared by
        the batch or [batch, nstages, nq] (every instance its own: the shape decides), one row per GRID POINT, and `active` with the
        same leading shape (isActive per grid point; None: active everywhere).  `costs.configuration_ref_table` fills both from
        the user's object.  q_ref = None removes the table: the constant q_ref of set_configuration_cost is in force again."""
        if q_ref is None:
            _chk(lib().rtoc_set_configuration_ref_table(self._h, None, None, 0, 0))
            return
        q = np.ascontiguousarray(q_ref, dtype=np.float64)
        nq = self.dims.nv + (1 if self.dims.np == 6 else 0)
        if q.ndim not in (2, 3) or q.shape[-1] != nq or (q.ndim == 3 and q.shape[0] != self.batch):
            raise ValueError("q_ref must be [nstages, %d] or [%d, nstages, %d], not %s" % (nq, self.batch, nq, q.shape))
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active) != 0, dtype=np.int32)
            if act.shape != q.shape[:-1]:
                raise ValueError("active must have the shape %s, not %s" % (q.shape[:-1], act.shape))
        _chk(lib().rtoc_set_configuration_ref_table(self._h, _dp(q), act.ctypes.data_as(C.POINTER(C.c_int)) if act is not None else None,
                                                    q.shape[-2], 1 if q.ndim == 3 else 0))

    def stage_costs(self):
        """rtoc_get_stage_costs: [batch, nstages] cost value of every grid point as the last evalKKT stored it"""
        out = np.zeros((self.batch, self.nstages))
        _chk(lib().rtoc_get_stage_costs(self._h, _dp(out), self.batch))
        return out

    def contact_eval_kkt(self):
        _chk(lib().rtoc_contact_eval_kkt(self._h))

    def set_task_costs(self, terms, per_instance=False):
        """rtoc_set_task_costs: `terms` = a list of robotoc_amd.costs.TaskSpace3DCost / CoMCost / TaskSpace6DCost (or TaskCost structs) shared by
        the batch, with per_instance a list of `batch` such lists; None or [] removes the terms"""
        from .costs import TaskCost
        if not terms:
            _chk(lib().rtoc_set_task_costs(self._h, None, 0, 0))
            return
        rows = [t for inst in terms for t in inst] if per_instance else list(terms)
        n = len(rows) // self.batch if per_instance else len(rows)
        if per_instance and any(len(inst) != n for inst in terms):
            raise ValueError("every instance needs the same number of terms")
        arr = (TaskCost * len(rows))(*[t if isinstance(t, TaskCost) else t.to_struct() for t in rows])
        _chk(lib().rtoc_set_task_costs(self._h, C.cast(arr, C.c_void_p), n, 1 if per_instance else 0))

    def set_task_ref_table(self, term, entries, per_instance=False):
        """rtoc_set_task_ref_table: the reference table of term `term` (ref_kind RTOC_REF_TABLE) -- `entries` = a
        costs.TaskRefEntry array with one entry per grid point (what a cost's `ref_table(grid_infos)` returns), with
        per_instance a list of `batch` such arrays"""
        from .costs import TaskRefEntry
        if per_instance:
            if len(entries) != self.batch:
                raise ValueError("a per-instance table needs one array per instance")
            n = len(entries[0])
            if any(len(e) != n for e in entries):
                raise ValueError("every instance needs a table of the same length")
            arr = (TaskRefEntry * (n * self.batch))(*[x for e in entries for x in e])
        else:
            n, arr = len(entries), (TaskRefEntry * len(entries))(*entries)
        _chk(lib().rtoc_set_task_ref_table(self._h, int(term), C.cast(arr, C.c_void_p), n, 1 if per_instance else 0))

    def set_task_ref_tables(self, terms, infos):
        """fills and uploads the table of every term of `terms` (the list given to set_task_costs, shared by the batch) whose
        reference is the user's object, asking it at the grid points `infos` (costs.grid_infos)"""
        for k, t in enumerate(terms):
            tab = t.ref_table(infos) if hasattr(t, "ref_table") else None
            if tab is not None:
                self.set_task_ref_table(k, tab)

    def set_contact_force_cost(self, cost, per_instance=False):
        """rtoc_set_contact_force_cost: `cost` = a robotoc_amd.costs.LocalContactForceCost (or ContactForceCost struct) shared by the
        batch, with per_instance a list of `batch` of them; None removes the term"""
        from .costs import ContactForceCost
        if cost is None:
            _chk(lib().rtoc_set_contact_force_cost(self._h, None, 0))
            return
        rows = list(cost) if per_instance else [cost]
        if per_instance and len(rows) != self.batch:
            raise ValueError("a per-instance force cost needs one term per instance")
        arr = (ContactForceCost * len(rows))(*[t if isinstance(t, ContactForceCost) else t.to_struct() for t in rows])
        _chk(lib().rtoc_set_contact_force_cost(self._h, C.cast(arr, C.c_void_p), 1 if per_instance else 0))

    def set_grid_times(self, t):
        """rtoc_set_grid_times: GridInfo::t of every grid point of a fixed grid"""
        t = np.ascontiguousarray(t, dtype=np.float64)
        _chk(lib().rtoc_set_grid_times(self._h, _dp(t), t.size))

    def grid_times(self):
        """rtoc_get_grid_times: [batch, nstages] grid times as rtoc_contact_eval_kkt uses them"""
        out = np.zeros((self.batch, self.nstages))
        _chk(lib().rtoc_get_grid_times(self._h, _dp(out), self.batch))
        return out

    def contact_update_solution(self, fraction_to_boundary_rule=0.995, want_kkt_error=True):
        out = np.zeros(self.batch) if want_kkt_error else None
        _chk(lib().rtoc_contact_update_solution(self._h, fraction_to_boundary_rule, _dp(out) if want_kkt_error else None,
                                                self.batch if want_kkt_error else 0))
        return out

    def set_initial_state(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        assert x0.shape == (self.batch, 2 * self.dims.nv + (1 if self.dims.np == 6 else 0))
        _chk(lib().rtoc_set_initial_state(self._h, _dp(x0), self.batch))

    def set_constraint_bounds(self, bounds, barrier_param=1.0e-3, fraction_to_boundary_rule=0.995):
        bounds = np.ascontiguousarray(bounds, dtype=np.float64)
        _chk(lib().rtoc_set_constraint_bounds(self._h, _dp(bounds), bounds.size, barrier_param, fraction_to_boundary_rule))

    def set_barrier_param(self, barrier_param=1.0e-3, fraction_to_boundary_rule=0.995):
        _chk(lib().rtoc_set_barrier_param(self._h, barrier_param, fraction_to_boundary_rule))

    def set_friction_coefficients(self, mu):
        """ContactStatus::frictionCoefficient per contact: switches the device-side evaluation of the friction-cone rows on"""
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        _chk(lib().rtoc_set_friction_coefficients(self._h, _dp(mu), mu.size))

    def set_wrench_cone_params(self, xy_mu):
        """[ncontacts][3] = sole half-extents X, Y and the friction coefficient: device-side evaluation of the wrench-cone rows"""
        xy_mu = np.ascontiguousarray(xy_mu, dtype=np.float64).reshape(-1, 3)
        _chk(lib().rtoc_set_wrench_cone_params(self._h, _dp(xy_mu), xy_mu.shape[0]))

    def contact_init_constraints(self):
        """OCPSolver::initConstraints for the rows evaluated on the device (joint limits with bounds, friction cones with mu)"""
        _chk(lib().rtoc_contact_init_constraints(self._h))

    def set_cone_jacobian(self, exact):
        """RTOC_OPT_CONE_JACOBIAN: dg/dq of the friction cones -- False (default): as the reference composes it (LOCAL-frame
        angular Jacobian x world-frame force); True: the derivative of R_wf(q) f"""
        _chk(lib().rtoc_set_option(self._h, OPT_CONE_JACOBIAN, int(bool(exact))))

    def set_linearize_fused(self, on):
        """RTOC_OPT_LINEARIZE_FUSED: rigid-body linearisation as one kernel (values recomputed per lane) instead of pre-pass + walk"""
        _chk(lib().rtoc_set_option(self._h, OPT_LINEARIZE_FUSED, int(bool(on))))

    def set_linearize_dofs_per_pass(self, dofs):
        """RTOC_OPT_LINEARIZE_DOFS_PER_PASS: tangent directions per pass of the rigid-body walk (0 = chosen per model)"""
        _chk(lib().rtoc_set_option(self._h, OPT_LINEARIZE_DOFS_PER_PASS, int(dofs)))

    def set_unconstr_dense(self, on):
        """RTOC_OPT_UNCONSTR_DENSE: the unconstrained recursion on materialised A, B (general kernels) instead of the structured one"""
        _chk(lib().rtoc_set_option(self._h, OPT_UNCONSTR_DENSE, int(bool(on))))

    def set_impact_cones(self, on):
        """RTOC_OPT_IMPACT_CONES: cone rows on impact grids (ImpactFrictionCone) or not"""
        _chk(lib().rtoc_set_option(self._h, OPT_IMPACT_CONES, int(bool(on))))

    def unconstr_init_constraints(self):
        _chk(lib().rtoc_unconstr_init_constraints(self._h))

    def linearize_state_equation(self):
        _chk(lib().rtoc_linearize_state_equation(self._h))

    def unconstr_eval_kkt(self, dt):
        _chk(lib().rtoc_unconstr_eval_kkt(self._h, dt))

    def unconstr_update_solution(self, dt, want_kkt_error=True):
        """rtoc_unconstr_update_solution; returns the KKT error of the iterate it linearised at ([batch]) or None"""
        out = np.zeros(self.batch) if want_kkt_error else None
        _chk(lib().rtoc_unconstr_update_solution(self._h, dt, _dp(out) if want_kkt_error else None, self.batch if want_kkt_error else 0))
        return out

    # ---- UnconstrParNMPCSolver on the device (include/rtoc_robot.h) ----
    def parnmpc_set_horizon(self, N):
        """rtoc_parnmpc_set_horizon: the records become the N stages of a ParNMPC horizon (every one with dynamics and rows)"""
        _chk(lib().rtoc_parnmpc_set_horizon(self._h, int(N)))
        self.nstages = int(N)

    def parnmpc_init_constraints(self):
        _chk(lib().rtoc_parnmpc_init_constraints(self._h))

    def parnmpc_init_backward_correction(self):
        _chk(lib().rtoc_parnmpc_init_backward_correction(self._h))

    def parnmpc_set_aux_mat(self, aux):
        """aux: [batch, N, 2nv, 2nv] (symmetric; stored column-major)"""
        nx = 2 * self.dims.nv
        aux = np.ascontiguousarray(np.swapaxes(np.asarray(aux, dtype=np.float64).reshape(self.batch, self.nstages, nx, nx), 2, 3))
        _chk(lib().rtoc_parnmpc_set_aux_mat(self._h, _dp(aux), self.batch))

    def parnmpc_get_aux_mat(self):
        """the auxiliary matrices [batch, N, 2nv, 2nv]"""
        nx = 2 * self.dims.nv
        out = np.empty((self.batch, self.nstages, nx, nx))
        _chk(lib().rtoc_parnmpc_get_aux_mat(self._h, _dp(out), self.batch))
        return np.ascontiguousarray(np.swapaxes(out, 2, 3))

    def parnmpc_eval_kkt(self, dt):
        _chk(lib().rtoc_parnmpc_eval_kkt(self._h, dt))

    def parnmpc_backward_correction(self, dt):
        _chk(lib().rtoc_parnmpc_backward_correction(self._h, dt))

    def parnmpc_update_solution(self, dt, want_kkt_error=True):
        """rtoc_parnmpc_update_solution; returns the KKT error of the iterate it linearised at ([batch]) or None"""
        out = np.zeros(self.batch) if want_kkt_error else None
        _chk(lib().rtoc_parnmpc_update_solution(self._h, dt, _dp(out) if want_kkt_error else None, self.batch if want_kkt_error else 0))
        return out

    def linearize_contact_dynamics(self, augment_residual=False):
        _chk(lib().rtoc_linearize_contact_dynamics(self._h, int(bool(augment_residual))))

    def kkt_error(self):
        """rtoc_kkt_error: sqrt of the squared KKT residual of every instance."""
        out = np.empty(self.batch, dtype=np.float64)
        _chk(lib().rtoc_kkt_error(self._h, _dp(out), self.batch))
        return out

    def save_stage_dump(self, path, buffers):
        """rtoc_save_stage_dump: `buffers` = iterable of RTOC_BUF_* indices."""
        mask = 0
        for b in buffers:
            mask |= 1 << b
        _chk(lib().rtoc_save_stage_dump(self._h, str(path).encode(), mask))

    def set_friction_cones(self, max_contacts, contact_dim=3):
        _chk(lib().rtoc_set_friction_cones(self._h, int(max_contacts), int(contact_dim)))

    def set_wrench_cones(self, max_contacts):
        """ContactWrenchCone rows (17 per active surface contact); replaces friction cones if set."""
        _chk(lib().rtoc_set_wrench_cones(self._h, int(max_contacts)))

    def unconstr_condense(self):
        _chk(lib().rtoc_unconstr_condense(self._h))

    def unconstr_expand(self, dt):
        _chk(lib().rtoc_unconstr_expand(self._h, dt))

    def unconstr_backward(self, dt):
        _chk(lib().rtoc_unconstr_backward(self._h, dt))

    def unconstr_forward(self, dt):
        _chk(lib().rtoc_unconstr_forward(self._h, dt))

    def expand(self, tau=0.995):
        _chk(lib().rtoc_expand(self._h, tau))

    def update(self):
        _chk(lib().rtoc_update(self._h))

    def status(self):
        out = (C.c_uint32 * self.batch)()
        _chk(lib().rtoc_status(self._h, out, self.batch))
        return np.frombuffer(out, dtype=np.uint32).copy()

    def clear_status(self):
        _chk(lib().rtoc_clear_status(self._h))

    def sync(self):
        _chk(lib().rtoc_sync(self._h))

    def gather_directions(self, nccl_comm, out_device_ptr):
        """rtoc_gather_directions: RCCL all-gather of RTOC_BUF_DIR of every rank into device memory of
        world_size * buffer_count(BUF_DIR) doubles; nccl_comm: ncclComm_t as an int / c_void_p."""
        _chk(lib().rtoc_gather_directions(self._h, C.c_void_p(nccl_comm if isinstance(nccl_comm, int) else nccl_comm.value),
                                          C.cast(C.c_void_p(out_device_ptr), C.POINTER(C.c_double))))

    def time_phase(self, phase, reps):
        ms = C.c_float()
        _chk(lib().rtoc_time_phase(self._h, phase, reps, C.byref(ms)))
        return ms.value

    # convenience shapes
    def shape(self, which):
        rl = getattr(self.L, which)
        return (self.batch, self.nstages, rl.stride)

    def upload_records(self, buffer, arr):
        """arr: [batch, nstages, stride] -> device layout [batch][max? no: nstages] (stride packed)."""
        assert arr.shape[1] == self.nstages
        self.upload(buffer, arr)

    def download_records(self, buffer, which):
        return self.download(buffer, self.shape(which))


class SolveOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("kkt_tol", C.c_double), ("sto_enabled", C.c_int), ("initial_sto_reg_iter", C.c_int),
                ("initial_sto_reg", C.c_double), ("kkt_tol_mesh", C.c_double), ("max_dt_mesh", C.c_double)]


_REG_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double)
_UPD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))
_REF_CB = C.CFUNCTYPE(C.c_int, C.c_void_p)


class SolveCallbacks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("set_sto_regularization", _REG_CB), ("update_solution", _UPD_CB), ("max_time_step", _UPD_CB),
                ("mesh_refinement", _REF_CB)]


class SolveStats(C.Structure):
    _fields_ = [("convergence", C.c_int), ("iter", C.c_int), ("num_mesh_refinements", C.c_int), ("mesh_refinement_iter", C.c_int * 64)]


def solve_loop(max_iter, kkt_tol, update_solution, sto_enabled=False, initial_sto_reg_iter=0, initial_sto_reg=0.0, kkt_tol_mesh=0.0,
               max_dt_mesh=0.0, set_sto_regularization=None, max_time_step=None, mesh_refinement=None):
    """rtoc_solve_loop (include/rtoc_robot.h): OCPSolver::solve's iteration schedule (ocp_solver.cpp:169-213), the one the C++ shell
    runs too.  update_solution() -> KKT error; max_time_step() -> float; set_sto_regularization(reg), mesh_refinement() -> None.
    Returns (convergence, iter, mesh_refinement_iter).  An exception raised by a callback aborts the loop and is re-raised."""
    pending = []

    def guard(fn):
        def run(*args):
            try:
                return fn(*args)
            except BaseException as e:   # (must not propagate through the C frame)
                pending.append(e)
                return -100
        return run

    def _upd(_, out):
        out[0] = float(update_solution())
        return 0

    def _mdt(_, out):
        out[0] = float(max_time_step())
        return 0

    def _reg(_, reg):
        set_sto_regularization(reg)
        return 0

    def _ref(_):
        mesh_refinement()
        return 0
    cb = SolveCallbacks(None, _REG_CB(guard(_reg)) if set_sto_regularization else _REG_CB(), _UPD_CB(guard(_upd)),
                        _UPD_CB(guard(_mdt)) if max_time_step else _UPD_CB(), _REF_CB(guard(_ref)) if mesh_refinement else _REF_CB())
    opt = SolveOptions(int(max_iter), float(kkt_tol), int(bool(sto_enabled)), int(initial_sto_reg_iter), float(initial_sto_reg),
                       float(kkt_tol_mesh), float(max_dt_mesh))
    st = SolveStats()
    L = lib()
    L.rtoc_solve_loop.argtypes = [C.POINTER(SolveOptions), C.POINTER(SolveCallbacks), C.POINTER(SolveStats)]
    rc = L.rtoc_solve_loop(C.byref(opt), C.byref(cb), C.byref(st))
    if pending:
        raise pending[0]
    _chk(rc)
    return bool(st.convergence), st.iter, [st.mesh_refinement_iter[k] for k in range(min(st.num_mesh_refinements, 64))]


def debug_profile(ctx):
    """Tuning aid: first call attaches the stamp buffer, later calls return [max_stages,32] int64."""
    L = lib()
    L.rtoc_debug_profile.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros((ctx.max_stages, 32), dtype=np.int64)
    _chk(L.rtoc_debug_profile(ctx._h, out.ctypes.data_as(C.c_void_p)))
    return out


class LinearizePlan(C.Structure):
    _fields_ = [("nlevels", C.c_int), ("nbranch", C.c_int), ("dofs_per_pass", C.c_int), ("npass", C.c_int), ("lds_bytes", C.c_int)]


def robot_model_plan(model, forced_dofs_per_pass=0):
    """rtoc_robot_model_plan: the storage plan and the passes rtoc_set_robot_model would give the tangent walk of `model`
    (host arithmetic: no device needed).  Returns (LinearizePlan, [bodies pass p visits])."""
    plan = LinearizePlan()
    masks = (C.c_ulonglong * 64)()
    lib().rtoc_robot_model_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _chk(lib().rtoc_robot_model_plan(C.byref(model), int(forced_dofs_per_pass), C.byref(plan), masks))
    return plan, [[i for i in range(model.njoints) if (masks[p] >> i) & 1] for p in range(plan.npass)]


def bandwidth_probe(device=0, nbytes=1 << 31):
    """rtoc_bandwidth_probe: (read GB/s, copy GB/s) of the library's own streaming kernels on `device`"""
    r, c = C.c_double(0.0), C.c_double(0.0)
    lib().rtoc_bandwidth_probe.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _chk(lib().rtoc_bandwidth_probe(int(device), int(nbytes), C.byref(r), C.byref(c)))
    return r.value, c.value


def wrench_cone_matrix(X, Y, mu):
    """rtoc_wrench_cone_matrix -> 17 x 6 array (ContactWrenchCone::computeCone)."""
    out = np.zeros(102)
    _chk(lib().rtoc_wrench_cone_matrix(X, Y, mu, _dp(out)))
    return out.reshape(6, 17).T.copy()
