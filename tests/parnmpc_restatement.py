"""numpy restatement of the reference's UnconstrParNMPC algorithm, line by line: the KKT-matrix inverter, the split backward
correction, the four correction passes with their lagged auxiliary matrices, and the backward-Euler stage.  The GPU tests hold
the HIP kernels to it; tests/test_parnmpc_restatement.py holds it to dense linear algebra.  Rigid-body terms come from the CPU
oracle (oracle.rbd_eval / oracle.rbd_linearize_cs).  Cited files are the reference's:
  inverter   include/robotoc/parnmpc/unconstr_kkt_matrix_inverter.hxx
  split      src/parnmpc/unconstr_split_backward_correction.cpp, include/robotoc/parnmpc/unconstr_split_backward_correction.hpp
  passes     src/parnmpc/unconstr_backward_correction.cpp
  stage      src/unconstr/parnmpc_intermediate_stage.cpp, parnmpc_terminal_stage.cpp, src/dynamics/unconstr_state_equation.cpp,
             src/dynamics/unconstr_dynamics.cpp
Variable order of a stage's KKT system: (lmd, gmm | a, q, v); H is over (a, q, v)."""
import numpy as np


def jacobian(nv, dt):
    """F = [[0, -I, dt I], [dt I, 0, -I]] over (a, q, v): d(Fq, Fv) of unconstr_state_equation.cpp:70-71"""
    I, Z = np.eye(nv), np.zeros((nv, nv))
    return np.block([[Z, -I, dt * I], [dt * I, Z, -I]])


def saddle_matrix(H, dt):
    """K = [[0, F], [F^T, H]], dense"""
    nv = H.shape[0] // 3
    F = jacobian(nv, dt)
    return np.block([[np.zeros((2 * nv, 2 * nv)), F], [F.T, H]])


def _llt_inverse(A):
    """llt.solve(Identity): Cholesky factor, two triangular solves"""
    L = np.linalg.cholesky(A)
    Y = np.linalg.solve(L, np.eye(A.shape[0]))
    return Y.T @ Y


def invert(dt, H):
    """UnconstrKKTMatrixInverter::invert (unconstr_kkt_matrix_inverter.hxx:39-79)"""
    nv = H.shape[0] // 3
    nx, nH, nk = 2 * nv, 3 * nv, 5 * nv
    Kinv = np.zeros((nk, nk))
    Kinv[nx:, nx:] = _llt_inverse(H)                                                   # :46-49
    FHinv = np.zeros((nx, nH))
    FHinv[:nv] = -Kinv[3 * nv:4 * nv, nx:] + dt * Kinv[4 * nv:, nx:]                   # :50-52
    FHinv[nv:] = dt * Kinv[nx:3 * nv, nx:] - Kinv[4 * nv:, nx:]                        # :53-55
    S = np.zeros((nx, nx))
    S[:nv, :nv] = -FHinv[:nv, nv:2 * nv] + dt * FHinv[:nv, 2 * nv:]                    # :56-58
    S[:nv, nv:] = dt * FHinv[:nv, :nv] - FHinv[:nv, 2 * nv:]                           # :59-61
    S[nv:, :nv] = -FHinv[nv:, nv:2 * nv] + dt * FHinv[nv:, 2 * nv:]                    # :62-64
    S[nv:, nv:] = dt * FHinv[nv:, :nv] - FHinv[nv:, 2 * nv:]                           # :65-67
    Kinv[:nx, :nx] = -_llt_inverse(S)                                                  # :68-71
    Kinv[:nx, nx:] = -Kinv[:nx, :nx] @ FHinv                                           # :72-73
    Kinv[nx:, :nx] = Kinv[:nx, nx:].T                                                  # :74-75
    Kinv[nx:, nx:] -= Kinv[:nx, nx:].T @ S @ Kinv[:nx, nx:]                            # :76-78
    return Kinv


def assemble_H(rec, aux_next=None):
    """H of coarseUpdate_impl (unconstr_split_backward_correction.hpp:168-171; the terminal overload .cpp:61-63 adds nothing)"""
    nv = rec["Qaa"].shape[0]
    H = np.zeros((3 * nv, 3 * nv))
    H[:nv, :nv] = rec["Qaa"]
    H[nv:, :nv] = rec["Qxa"]
    H[:nv, nv:] = rec["Qxa"].T       # (Eigen's LLT reads the lower triangle: the mirror image is what it factorises)
    H[nv:, nv:] = rec["Qxx"].T
    if aux_next is not None:
        H[nv:, nv:] += aux_next
    return H


class SplitCorrector:
    """UnconstrSplitBackwardCorrection of one stage; a solution vector is (lmd, gmm, a, q, v)"""

    def coarse_update(self, dt, rec, s, aux_next=None):
        nv = rec["Qaa"].shape[0]
        self.nv = nv
        self.Kinv = invert(dt, assemble_H(rec, aux_next))                              # .hpp:172
        res = np.concatenate([rec["Fx"], rec["la"], rec["lx"]])                        # .hpp:173-175
        self.x_res = np.zeros(2 * nv)
        return s - self.Kinv @ res                                                     # .hpp:176-181

    def aux_mat(self):
        return self.Kinv[:2 * self.nv, :2 * self.nv]                                   # .cpp:77-80

    def backward_serial(self, s_next, s_new_next, s_new):
        nv = self.nv
        self.x_res = (s_new_next - s_next)[:2 * nv].copy()                             # .cpp:86-87
        s_new[:2 * nv] -= self.Kinv[:2 * nv, 3 * nv:] @ self.x_res                     # .cpp:88-90

    def backward_parallel(self, s_new):
        s_new[2 * self.nv:] -= self.Kinv[2 * self.nv:, 3 * self.nv:] @ self.x_res      # .cpp:96-100

    def forward_serial(self, s_prev, s_new_prev, s_new):
        nv = self.nv
        self.x_res = (s_new_prev - s_prev)[3 * nv:].copy()                             # .cpp:107-108
        s_new[3 * nv:] -= self.Kinv[3 * nv:, :2 * nv] @ self.x_res                     # .cpp:109-111

    def forward_parallel(self, s_new):
        s_new[:3 * self.nv] -= self.Kinv[:3 * self.nv, :2 * self.nv] @ self.x_res      # .cpp:117-121


def backward_correction(dt, recs, s, aux):
    """coarseUpdate + backwardCorrection of one instance (unconstr_backward_correction.cpp:154-228) on CONDENSED records.
    recs[i]: dict Qaa, Qxa, Qxx, Fx, la, lx; s: [N, 5 nv]; aux: [N, 2nv, 2nv].  Returns (d [N, 5 nv], the next aux, the inverses)."""
    N = len(recs)
    cor = [SplitCorrector() for _ in range(N)]
    s_new = np.zeros_like(s)
    for i in range(N):                                                                 # :161-183
        s_new[i] = cor[i].coarse_update(dt, recs[i], s[i], aux[i + 1] if i < N - 1 else None)
    for i in range(N - 2, -1, -1):                                                     # :196-198
        cor[i].backward_serial(s[i + 1], s_new[i + 1], s_new[i])
    for i in range(N - 2, -1, -1):                                                     # :200-202
        cor[i].backward_parallel(s_new[i])
    for i in range(1, N):                                                              # :203-205
        cor[i].forward_serial(s[i - 1], s_new[i - 1], s_new[i])
    aux_new = aux.copy()
    for i in range(1, N):                                                              # :207-211
        cor[i].forward_parallel(s_new[i])
        aux_new[i] = -cor[i].aux_mat()
    return s_new - s, aux_new, [c.Kinv for c in cor]                                   # computeDirection (.cpp:125-133)


# ---- the backward-Euler stage ----
def eval_stage(oracle, m, cost, dt, q_prev, v_prev, s, s_next):
    """ParNMPCIntermediateStage / ParNMPCTerminalStage::evalKKT up to the condensations (parnmpc_terminal_stage.cpp:84-105), without
    inequality rows.  s, s_next: dicts q, v, a, u, lmd, gmm, beta; s_next None on the last stage.  Fields named as the device
    records hold them: la is the reference's la (KKT.lu), lu its lu (CDD.la)."""
    nv = m.nv
    z = np.zeros(0)
    q, v, a, u, lmd, gmm, beta = (s[k] for k in ("q", "v", "a", "u", "lmd", "gmm", "beta"))
    last = s_next is None
    # quadratizeStageCost (configuration_space_cost.cpp:274-324), scaled by dt
    lq = dt * cost["q_weight"] * (q - cost["q_ref"])
    lv = dt * cost["v_weight"] * (v - cost["v_ref"])
    la = dt * cost["a_weight"] * a
    lu = dt * cost["u_weight"] * (u - cost["u_ref"])
    Qqq, Qvv, Qaa, Quu = dt * cost["q_weight"], dt * cost["v_weight"], dt * cost["a_weight"], dt * cost["u_weight"]
    if last:                                                                           # + quadratizeTerminalCost (:88-93)
        lq = lq + cost["q_weight_terminal"] * (q - cost["q_ref"])
        lv = lv + cost["v_weight_terminal"] * (v - cost["v_ref"])
        Qqq, Qvv = Qqq + cost["q_weight_terminal"], Qvv + cost["v_weight_terminal"]
    Fx = np.concatenate([q_prev - q + dt * v, v_prev - v + dt * a])                    # unconstr_state_equation.cpp:70-71
    if last:                                                                           # :50-52
        lq = lq - lmd
    else:                                                                              # :36-38
        lq = lq + s_next["lmd"] - lmd
    lv = lv + dt * lmd - gmm + (0.0 if last else s_next["gmm"])
    la = la + dt * gmm
    ID = oracle.rbd_eval(m, 0, q, v, a, z, u, 0, z)                                    # unconstr_dynamics.cpp:53-64
    Dq, Dv, Da = oracle.rbd_linearize_cs(m, 0, q, v, a, z, u, 0, z)
    lq = lq + dt * Dq.T @ beta
    lv = lv + dt * Dv.T @ beta
    la = la + dt * Da.T @ beta
    lu = lu - dt * beta
    lx = np.concatenate([lq, lv])
    err = Fx @ Fx + lx @ lx + la @ la + lu @ lu + ID @ ID                              # split_kkt_residual.hxx:90-104 + UnconstrOCPData::KKTError
    return dict(Fx=Fx, lx=lx, la=la, lu=lu, Qxx_diag=np.concatenate([Qqq, Qvv]), Qaa_diag=Qaa, Quu_diag=Quu, ID=ID, Dq=Dq, Dv=Dv, Da=Da,
                kkt_error=err)


def condense_stage(st):
    """UnconstrDynamics::condenseUnconstrDynamics (unconstr_dynamics.cpp:67-88) -> the record backward_correction reads"""
    W = st["Quu_diag"]
    Dq, Dv, Da = st["Dq"], st["Dv"], st["Da"]
    nv = Dq.shape[0]
    luc = st["lu"] + W * st["ID"]                                                      # :70-71
    lx = st["lx"] + np.concatenate([Dq.T @ luc, Dv.T @ luc])                           # :72-73
    la = st["la"] + Da.T @ luc                                                         # :74
    Qxx = np.diag(st["Qxx_diag"])
    Qxx[:nv, :nv] += Dq.T @ (W[:, None] * Dq)                                          # :79
    Qxx[:nv, nv:] += Dq.T @ (W[:, None] * Dv)                                          # :80
    Qxx[nv:, :nv] = Qxx[:nv, nv:].T                                                    # :81
    Qxx[nv:, nv:] += Dv.T @ (W[:, None] * Dv)                                          # :82
    Qaa = np.diag(st["Qaa_diag"]) + Da.T @ (W[:, None] * Da)                           # :83
    Qxa = np.vstack([Dq.T @ (W[:, None] * Da), Dv.T @ (W[:, None] * Da)])              # :86-87
    return dict(Qaa=Qaa, Qxa=Qxa, Qxx=Qxx, Fx=st["Fx"], la=la, lx=lx)


def expand_stage(st, dt, d):
    """expandPrimal / expandDual (unconstr_dynamics.cpp:91-104): du, dbeta from d = (dlmd, dgmm, da, dq, dv)"""
    nv = st["Dq"].shape[0]
    da, dq, dv = d[2 * nv:3 * nv], d[3 * nv:4 * nv], d[4 * nv:]
    du = st["ID"] + st["Dq"] @ dq + st["Dv"] @ dv + st["Da"] @ da
    dbeta = (st["lu"] + st["Quu_diag"] * du) / dt
    return du, dbeta


FIELDS = ("lmd", "gmm", "a", "q", "v")


def pack(sol_i):
    return np.concatenate([sol_i[k] for k in FIELDS])


def iterate(oracle, m, cost, dt, q0, v0, sol, aux):
    """UnconstrParNMPCSolver::updateSolution (unconstr_parnmpc_solver.cpp:97-119) without inequality rows, step sizes 1.
    sol: list of N dicts (updated in place); returns (sqrt of the KKT error of the iterate it linearised at, the next aux)."""
    N, nv = len(sol), m.nv
    stages = [eval_stage(oracle, m, cost, dt, q0 if i == 0 else sol[i - 1]["q"], v0 if i == 0 else sol[i - 1]["v"], sol[i],
                         sol[i + 1] if i < N - 1 else None) for i in range(N)]
    err = np.sqrt(sum(st["kkt_error"] for st in stages))                               # :236-238
    recs = [condense_stage(st) for st in stages]
    s = np.array([pack(x) for x in sol])
    d, aux_new, _ = backward_correction(dt, recs, s, aux)
    for i in range(N):
        du, dbeta = expand_stage(stages[i], dt, d[i])
        for k, name in enumerate(FIELDS):                                              # SplitSolution::integrate
            sol[i][name] = sol[i][name] + d[i][k * nv:(k + 1) * nv]
        sol[i]["u"] = sol[i]["u"] + du
        sol[i]["beta"] = sol[i]["beta"] + dbeta
    return err, aux_new


def init_aux(cost, N):
    """initAuxMat (unconstr_backward_correction.cpp:57-71): every aux matrix is the terminal-cost Hessian"""
    return np.array([np.diag(np.concatenate([cost["q_weight_terminal"], cost["v_weight_terminal"]]))] * N)


def reference_test_problem(nv=7):
    """cost and initial state of the reference's test/solver/unconstr_parnmpc_solver_test.cpp (N = 20, T = 1)"""
    q_ref = np.array([0, np.pi / 2, 0, np.pi / 2, 0, np.pi / 2, 0])
    cost = dict(q_ref=q_ref, v_ref=np.zeros(nv), u_ref=np.zeros(nv), q_weight=np.full(nv, 10.0), v_weight=np.full(nv, 0.01),
                a_weight=np.full(nv, 0.01), u_weight=np.zeros(nv), q_weight_terminal=np.full(nv, 10.0),
                v_weight_terminal=np.full(nv, 0.01))
    q0 = np.array([np.pi / 2, 0, np.pi / 2, 0, np.pi / 2, 0, np.pi / 2])
    return cost, q0, np.zeros(nv), 20, 1.0
