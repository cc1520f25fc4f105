"""Every function of the C ABI (include/rtoc.h, include/rtoc_robot.h), classified by what it means for RTOC_OPT_GRAPH:

  mutator  changes context state a captured launch sequence may have frozen -- it names the case or cases of
           tests/test_graph_staleness_gpu.py that hold a replay to the plain launches after it ("test_name" or "test_name[case]");
  launch   runs kernels (or a copy) on the records and changes no configuration;
  query    download, get, count, or a function without a context.

tests/test_graph_mutators.py (CPU) fails when a declared function is missing here or listed twice, when an RTOC_OPT_* has no option
case, and when a case named here does not exist: a new setter or option is classified and given a case before the suite is green.
DESIGN.md ("RTOC_OPT_GRAPH: what must bump the epoch") states the rule the cases check."""

CL = "test_c_closed_loop[%s]"

MUTATORS = {
    # ---- rtoc.h
    "rtoc_create": ["test_r_graph_option_off_on_off_on"],            # every twin is built through it
    "rtoc_destroy": ["test_r_clone"],                                 # the clone destroyed beside the original
    "rtoc_clone": ["test_r_clone"],
    "rtoc_load_stage_dump": ["test_r_stage_dump_round_trip"],
    "rtoc_set_grid": ["test_r_set_grid", "test_s_sto_set_problem"],
    "rtoc_set_stream": ["test_r_set_stream"],
    "rtoc_set_option": ["test_r_option", "test_r_graph_option_off_on_off_on", "test_s_max_dts0", "test_w_backward_register"],
    "rtoc_upload": ["test_r_first_upload_of_the_solution", "test_r_fxx_verdict_flips"],
    "rtoc_device_ptr": ["test_r_device_ptr_creates_and_exposes"],
    "rtoc_bind": ["test_r_bind_and_rebind"],
    "rtoc_set_constraint_rows": ["test_r_set_constraint_rows", "test_r_set_constraint_rows_from_none"],
    "rtoc_set_friction_cones": ["test_r_set_friction_cones"],
    "rtoc_set_wrench_cones": ["test_c_wrench_cones_and_their_params", "test_r_set_wrench_cones_refused_leaves_the_sequence"],
    "rtoc_sto_set_problem": ["test_s_sto_set_problem", "test_s_sto_iterates"],
    "rtoc_sto_set_regularization": ["test_s_sto_scalars_and_cost_terms"],
    "rtoc_sto_set_cost_terms": ["test_s_sto_scalars_and_cost_terms"],
    "rtoc_sto_set_slack_dual": ["test_s_sto_set_slack_dual"],
    "rtoc_newton_iteration": ["test_r_new_tau_and_kkt_tol"],          # its two scalar arguments are part of the graph's key
    # ---- rtoc_robot.h: what rtoc_contact_eval_kkt reads, ahead of the captured iteration
    "rtoc_set_robot_model": [CL % "set_robot_model"],
    "rtoc_set_contact_schedule": [CL % "set_contact_schedule"],
    "rtoc_set_contact_placements": [CL % "set_contact_placements"],
    "rtoc_hold_contact_placements": [CL % "hold_contact_placements"],
    "rtoc_set_foot_step_planner": [CL % "foot_step_tick"],
    "rtoc_foot_step_place": [CL % "foot_step_tick"],
    "rtoc_foot_step_refs": [CL % "foot_step_tick"],
    "rtoc_set_task_costs": [CL % "task_costs"],
    "rtoc_set_grid_times": [CL % "task_costs"],
    "rtoc_set_task_ref_table": [CL % "task_costs"],
    "rtoc_set_contact_force_cost": [CL % "set_contact_force_cost"],
    "rtoc_set_barrier_param": [CL % "set_barrier_param"],
    "rtoc_set_friction_coefficients": [CL % "set_friction_coefficients"],
    "rtoc_set_wrench_cone_params": ["test_c_wrench_cones_and_their_params"],
    "rtoc_set_configuration_cost": [CL % "set_configuration_cost"],
    "rtoc_set_configuration_ref_table": [CL % "set_configuration_ref_table"],
    "rtoc_set_initial_state": [CL % "set_initial_state"],
    "rtoc_set_constraint_bounds": [CL % "set_constraint_bounds"],
    "rtoc_set_line_search": ["test_c_line_search_on_and_off", "test_inert_unconstr_update_solution"],
    "rtoc_set_line_search_method": ["test_c_line_search_on_and_off"],
    "rtoc_solution_store": [CL % "solution_store", "test_c_solution_interpolate_is_a_launch"],
    "rtoc_solution_forget": [CL % "solution_store"],
    "rtoc_parnmpc_set_horizon": ["test_inert_parnmpc"],
    "rtoc_parnmpc_set_aux_mat": ["test_inert_parnmpc"],
    # ---- the paths that are not graphed, listed here so that each keeps a case: one plain-vs-graph run, equal results, and the
    # replay counter does not move (RTOC_OPT_GRAPH is inert there)
    "rtoc_unconstr_update_solution": ["test_inert_unconstr_update_solution"],
    "rtoc_parnmpc_update_solution": ["test_inert_parnmpc"],
    "rtoc_contact_line_search": ["test_c_line_search_on_and_off"],   # the line-search iteration inside rtoc_newton_iteration
}

# entry points outside the two headers that change what a captured sequence froze
UNDECLARED_MUTATORS = {
    "rtoc_debug_profile": ["test_r_debug_profile_attach"],
}

LAUNCHES = [
    "rtoc_condense", "rtoc_riccati_backward", "rtoc_riccati_forward", "rtoc_riccati_sweep", "rtoc_unconstr_backward",
    "rtoc_unconstr_forward", "rtoc_unconstr_condense", "rtoc_unconstr_expand", "rtoc_expand", "rtoc_update",
    "rtoc_correct_state_equation", "rtoc_correct_costate_direction", "rtoc_compute_initial_state_direction",
    "rtoc_check_fxx_structure", "rtoc_clear_status", "rtoc_time_phase", "rtoc_sto_eval_kkt", "rtoc_sto_init_constraints",
    "rtoc_sto_correct_time_steps", "rtoc_sto_eval_kkt_device", "rtoc_sto_compute_step_sizes", "rtoc_sto_integrate_solution",
    "rtoc_line_search_filter", "rtoc_line_search_clear", "rtoc_integrate_solution", "rtoc_gather_directions",
    "rtoc_foot_step_planner_init", "rtoc_foot_step_plan", "rtoc_linearize_contact_dynamics", "rtoc_contact_eval_kkt",
    "rtoc_contact_init_constraints", "rtoc_contact_update_solution", "rtoc_solution_interpolate", "rtoc_contact_eval_ocp",
    "rtoc_linearize_state_equation", "rtoc_unconstr_eval_kkt", "rtoc_unconstr_init_constraints",
    "rtoc_parnmpc_init_constraints", "rtoc_parnmpc_init_backward_correction", "rtoc_parnmpc_eval_kkt",
    "rtoc_parnmpc_backward_correction", "rtoc_control_policy", "rtoc_control_input",
]

QUERIES = [
    "rtoc_version", "rtoc_device_count", "rtoc_bandwidth_probe", "rtoc_dims_supported", "rtoc_get_layout", "rtoc_get_option",
    "rtoc_download", "rtoc_buffer_count", "rtoc_wrench_cone_matrix", "rtoc_status", "rtoc_sync", "rtoc_kkt_error",
    "rtoc_sto_get_event_times", "rtoc_sto_get_time_steps", "rtoc_sto_get_constraint_data", "rtoc_sto_get_kkt_terms",
    "rtoc_graph_replay_count", "rtoc_converged_count", "rtoc_save_stage_dump", "rtoc_error_string", "rtoc_robot_model_plan",
    "rtoc_get_contact_placements", "rtoc_contact_frame_placements", "rtoc_foot_step_plan_get", "rtoc_get_task_ref_table",
    "rtoc_get_grid_times", "rtoc_solve_loop", "rtoc_solution_stored", "rtoc_get_stage_costs", "rtoc_line_search_merit_terms",
    "rtoc_line_search_trials", "rtoc_get_configuration_ref_table", "rtoc_parnmpc_get_aux_mat",
]

# every RTOC_OPT_* of the header -> its option case
OPTION_CASES = {
    "RTOC_OPT_WRITEBACK_KKT": "test_r_option[writeback_kkt]",
    "RTOC_OPT_MAX_DTS0": "test_s_max_dts0",
    "RTOC_OPT_BACKWARD_WAVES": "test_r_option[backward_waves]",
    "RTOC_OPT_CONTACT_INV_DAMPING": "test_r_option[contact_inv_damping]",
    "RTOC_OPT_SWEEP_CHUNKS": "test_r_option[sweep_chunks]",
    "RTOC_OPT_CONDENSE_SPLIT": "test_r_option[condense_split]",
    "RTOC_OPT_BACKWARD_SCAN": "test_r_option[backward_scan]",
    "RTOC_OPT_CONDENSE_KEEP_QAF": "test_r_option[condense_keep_qaf]",
    "RTOC_OPT_FXX_STRUCTURE": "test_r_option[fxx_structure]",
    "RTOC_OPT_GRAPH": "test_r_graph_option_off_on_off_on",
    "RTOC_OPT_CONE_JACOBIAN": CL % "cone_jacobian",
    "RTOC_OPT_LINEARIZE_DOFS_PER_PASS": CL % "linearize_dofs_per_pass",
    "RTOC_OPT_LINEARIZE_FUSED": CL % "linearize_fused",
    "RTOC_OPT_UNCONSTR_DENSE": "test_inert_unconstr_update_solution",
    "RTOC_OPT_IMPACT_CONES": "test_r_option[impact_cones]",
    "RTOC_OPT_BACKWARD_REGISTER": "test_r_option[backward_register]",
    "RTOC_OPT_CONDENSE_REGISTER": "test_r_option[condense_register]",
    "RTOC_OPT_SWITCHING_TRANSPORT": CL % "switching_transport",
}


def classes():
    """{function: class} over the three classes; a function listed twice raises"""
    out = {}
    for cls, names in (("mutator", list(MUTATORS)), ("launch", LAUNCHES), ("query", QUERIES)):
        for n in names:
            if n in out:
                raise ValueError("%s is classified twice (%s, %s)" % (n, out[n], cls))
            out[n] = cls
    return out


def named_cases():
    """every case a mutator or an option names"""
    out = set(OPTION_CASES.values())
    for cases in list(MUTATORS.values()) + list(UNDECLARED_MUTATORS.values()):
        out.update(cases)
    return sorted(out)
