"""One control tick of a batched trot MPC's planning at the bench size (ANYmal trot grid of bench.py, `batch` instances), for the record:
  * on the device: rtoc_foot_step_plan + rtoc_foot_step_place + rtoc_foot_step_refs (Raibert mode, every instance its own command);
  * the host path it replaces: the numpy restatement of TrotFootStepPlanner and the three MPCPeriodic references
    (tests/foot_step_planner_restatement.py) in a loop over the instances, kinematics by RobotModel.frame_placement and the
    restated centre of mass, then the three per-instance uploads (rtoc_set_contact_placements, rtoc_set_task_ref_table x 5,
    rtoc_set_configuration_ref_table).  The loop is timed over the first `host_instances` instances and scaled to the batch (the
    figure says so); the uploads are timed at the full batch.
Wall clock around `reps` asynchronous ticks, synchronised once, after a warm-up; three rounds each.
With --gait the plan alone is timed instead, per gait named (trot, crawl, pace, flying_trot, or all): rtoc_foot_step_plan -- the
kinematics launch and foot_step_plan_kernel -- at the gait's own swing status, 200 asynchronous calls synchronised once, five
rounds; the host path is left out.  A trot leaves the struct's gait member alone, so the same file times a library from before
the member had a meaning.
Usage: foot_step_planner_bench.py [batch] [out.json] [host_instances] [--gait NAME[,NAME...]]"""
import json
import os
import sys
import time

gaits = None
if "--gait" in sys.argv:
    at = sys.argv.index("--gait")
    gaits = sys.argv[at + 1].split(",")
    del sys.argv[at:at + 2]
    if gaits == ["all"]:
        gaits = ["trot", "crawl", "pace", "flying_trot"]
    GAIT_STATUS = {"trot": (0, 0b1001), "crawl": (1, 0b0111), "pace": (2, 0b0011), "flying_trot": (3, 0b1001)}   # RTOC_GAIT_*, a swing status
    if any(g not in GAIT_STATUS for g in gaits):
        sys.exit("--gait: trot, crawl, pace, flying_trot or all")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import foot_step_planner_restatement as fsr
from task_cost_restatement import com as com_restated
from robotoc_amd import capi, problems as pr, robot_model as rm
from robotoc_amd.costs import TaskCost, TaskRefEntry
from robotoc_amd.grid import ANYMAL_Q_STANDING, ANYMAL_TROT_IMPACT_MASKS, ANYMAL_TROT_PHASE_MASKS, contact_masks
from robotoc_amd.types import GRID_IMPACT, GRID_LIFT

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
host_n = min(batch, int(sys.argv[3]) if len(sys.argv) > 3 else 256)
m = rm.load_named("anymal")
dims, grids, _ = pr.config_anymal_trot()
n = len(grids)
phase, t, p, now = [], [], 0, 0.0
for g in grids:
    if g.type in (GRID_IMPACT, GRID_LIFT):
        p += 1
    phase.append(p)
    t.append(now)
    now += g.dt
phase, t = np.array(phase, dtype=np.int32), np.array(t)
masks = ANYMAL_TROT_PHASE_MASKS
nphases = len(masks)
assert phase.max() == nphases - 1
SWING, STANCE, GAIN, NPH, START, HEIGHT = 0.2, 0.1, 0.7, 2, 0.05, 0.08

ctx = capi.Context(dims, n, batch, 0)
ctx.set_grid(grids)
ctx.set_robot_model(m)
ctx.set_contact_schedule(contact_masks(grids, masks, ANYMAL_TROT_IMPACT_MASKS))
ctx.set_grid_times(t)
terms = []
for k in range(5):
    c = TaskCost()
    c.kind, c.ref_kind = (0 if k < 4 else 1), 3
    if k < 4:
        c.frame_parent = m.contact_parent[k]
        c.frame_p[:] = list(m.contact_p[k])
    c.weight[:] = [1.0e3] * 3
    terms.append(c)
ctx.set_task_costs(terms)
rng = np.random.default_rng(0)
x0 = np.zeros((batch, m.nq + m.nv))
x0[:, :m.nq] = ANYMAL_Q_STANDING
x0[:, 0:2] = rng.uniform(-5, 5, (batch, 2))
yaw = rng.uniform(-3, 3, batch)
x0[:, 5], x0[:, 6] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
x0[:, m.nq:m.nq + 3] = rng.uniform(-0.5, 0.5, (batch, 3))
vcmd = np.zeros((batch, 3))
vcmd[:, :2] = rng.uniform(-1, 1, (batch, 2))
yaw_rate = rng.uniform(-1, 1, batch)
ctx.set_initial_state(x0)
structs = []
for b in range(batch):
    s = capi.FootStepPlanner()
    s.mode, s.projection = capi.FOOT_STEP_RAIBERT, capi.PROJECT_YAW
    s.swing_time, s.stance_time, s.gain = SWING, STANCE, GAIN
    s.vcom_cmd[:], s.yaw_rate_cmd = list(vcmd[b]), float(yaw_rate[b])
    structs.append(s)
if gaits is not None:
    # ---- the plan alone, per gait ----
    out = {"batch": batch, "contact_phases": nphases, "reps": 200, "plan_ms": {}, "plans_finite": {}}
    for gait in gaits:
        gait_id, status = GAIT_STATUS[gait]
        for s in structs:
            if gait_id or hasattr(s, "gait"):
                s.gait = gait_id
        ctx.set_foot_step_planner(structs)
        ctx.foot_step_planner_init()
        ctx.foot_step_plan(0.0, 0b1111, nphases)
        tick_t = [0.0]

        def plan_alone():
            tick_t[0] += 0.0025
            ctx.foot_step_plan(tick_t[0], status, nphases)

        rounds = []
        for rnd in range(5):
            for _ in range(10):
                plan_alone()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(out["reps"]):
                plan_alone()
            ctx.sync()
            rounds.append((time.perf_counter() - t0) / out["reps"] * 1e3)
        out["plan_ms"][gait] = rounds
        out["plans_finite"][gait] = bool(ctx.foot_step_plan_get()["ok"].all())
    ctx.close()
    print(json.dumps(out))
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        json.dump(out, open(sys.argv[2], "w"), indent=1)
    sys.exit(0)
ctx.set_foot_step_planner(structs)
ctx.foot_step_planner_init()
refs = capi.FootStepRefs()
refs.foot_term[:] = (0, 1, 2, 3)
refs.com_term, refs.configuration = 4, 1
for k in range(4):
    refs.swing_height[k], refs.swing_start_time[k], refs.period_swing[k], refs.period_stance[k] = HEIGHT, START, SWING, SWING + 2 * STANCE
    refs.swing_num_phases_in_period[k] = NPH
refs.com_swing_start_time, refs.com_period_active, refs.com_period_inactive, refs.com_num_phases_in_period = START, SWING, STANCE, NPH
refs.q_swing_start_time, refs.q_period_active, refs.q_period_inactive, refs.q_num_phases_in_period = START, SWING, STANCE, NPH
tick_t = [0.0]


def device_tick():
    tick_t[0] += 0.0025
    ctx.foot_step_plan(tick_t[0], 0b1111, nphases)
    ctx.foot_step_place(phase)
    ctx.foot_step_refs(refs, phase, masks)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


out = {"batch": batch, "grid_points": n, "contact_phases": nphases, "host_instances": host_n, "device_tick_ms": [], "host_loop_ms_scaled_to_batch": [],
       "host_uploads_ms": []}
for rnd in range(3):
    out["device_tick_ms"].append(timed(device_tick, 20))
plan = ctx.foot_step_plan_get()
out["plans_finite"] = bool(plan["ok"].all())

# ---- the host path: the restatement per instance, then the three uploads ----
planners = []
for b in range(host_n):
    pl = fsr.TrotFootStepPlanner(yaw_projection=True)
    pl.set_raibert_gait_pattern(vcmd[b], yaw_rate[b], SWING, STANCE, GAIN)
    q = x0[b, :m.nq]
    pl.init(q, np.array([m.frame_placement(q, c)[1] for c in range(4)]), com_restated(m, q))
    planners.append(pl)
foot_par = (HEIGHT, START, SWING, SWING + 2 * STANCE, NPH)
par = (START, SWING, STANCE, NPH)
pos_tab, q_tab = np.zeros((host_n, n, 4, 3)), np.zeros((host_n, n, m.nq))
ref_tab = [[(TaskRefEntry * n)() for _ in range(host_n)] for _ in range(5)]
for rnd in range(3):
    t0 = time.perf_counter()
    for b, pl in enumerate(planners):
        q = x0[b, :m.nq]
        feet = np.array([m.frame_placement(q, c)[1] for c in range(4)])
        pl.plan(0.1 * (rnd + 1), feet, x0[b, m.nq:], 0b1111, nphases)
        P = np.array([pl.contact_positions(s) for s in range(pl.size())])
        C = np.array([pl.com(s) for s in range(pl.size())])
        R = np.array([pl.R(s) for s in range(pl.size())])
        for i in range(n):
            pos_tab[b, i] = P[phase[i] + 1]
            for k in range(4):
                x, a = fsr.swing_foot_ref(P, k, masks, t[i], phase[i], *foot_par)
                e = ref_tab[k][b][i]
                e.p[:], e.active = list(x), int(a)
            x, a = fsr.com_ref(C, masks, t[i], phase[i], *par)
            e = ref_tab[4][b][i]
            e.p[:], e.active = list(x), int(a)
            q_tab[b, i] = fsr.configuration_ref(q, R, masks, t[i], phase[i], *par)[0]
    out["host_loop_ms_scaled_to_batch"].append((time.perf_counter() - t0) * 1e3 * batch / host_n)
reps = -(-batch // host_n)
pos_full = np.ascontiguousarray(np.tile(pos_tab, (reps, 1, 1, 1))[:batch])
q_full = np.ascontiguousarray(np.tile(q_tab, (reps, 1, 1))[:batch])
ref_full = [[ref_tab[k][b % host_n] for b in range(batch)] for k in range(5)]
for rnd in range(3):
    t0 = time.perf_counter()
    ctx.set_contact_placements(pos_full)
    for k in range(5):
        ctx.set_task_ref_table(k, ref_full[k], per_instance=True)
    ctx.set_configuration_ref_table(q_full)
    ctx.sync()
    out["host_uploads_ms"].append((time.perf_counter() - t0) * 1e3)
ctx.close()
print(json.dumps(out))
if len(sys.argv) > 2:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    json.dump(out, open(sys.argv[2], "w"), indent=1)
