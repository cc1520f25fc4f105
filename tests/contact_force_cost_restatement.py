"""numpy restatement of LocalContactForceCost (reference src/cost/local_contact_force_cost.cpp), written from reading it: the
yardstick of tests/test_contact_force_cost.py, itself pinned by finite differences and hand-computed cases in
tests/test_contact_force_cost_host.py.

f is the compacted stack of the active contacts' forces, as SplitSolution::f_stack and the SOL record's `f` field hold it:
3 rows per active point contact, 6 per active surface contact, in contact order."""
import numpy as np

CONTACT_POINT, CONTACT_SURFACE = 0, 1


def offsets(active_mask, contact_types):
    """o_i of every contact (None where it is inactive) and the rows of the stack"""
    out, o = [], 0
    for i, t in enumerate(contact_types):
        if (int(active_mask) >> i) & 1:
            out.append(o)
            o += 6 if t == CONTACT_SURFACE else 3
        else:
            out.append(None)
    return out, o


def _arrays(cost, kind):
    ref, w = (cost.fi_ref, cost.fi_weight) if kind == "impact" else (cost.f_ref, cost.f_weight)
    return np.array([list(r) for r in ref], dtype=float), np.array([list(r) for r in w], dtype=float)


def value(f, active_mask, contact_types, cost, kind, scale):
    """evalStageCost (:81-95, scale = dt) / evalImpactCost (:169-181, scale = 1) / evalTerminalCost (:147-152)"""
    if kind == "terminal":
        return 0.0
    ref, w = _arrays(cost, kind)
    offs, _ = offsets(active_mask, contact_types)
    l = 0.0
    for i, o in enumerate(offs):
        if o is not None:
            d = np.asarray(f[o:o + 3], dtype=float) - ref[i]
            l += float(np.sum(w[i] * d * d))
    return 0.5 * scale * l


def stage_terms(f, active_mask, contact_types, cost, kind, scale):
    """what the term adds at one grid point: lf, diag(Qff), hf, h (all of the length of f; hf and h zero except on "stage"
    grid points) and the cost value.  kind: "stage" (intermediate / lift; scale = dt), "impact" (scale = 1), "terminal"."""
    n = len(f)
    lf, qff, hf, h = np.zeros(n), np.zeros(n), np.zeros(n), 0.0
    if kind == "terminal":
        return lf, qff, hf, h, 0.0
    ref, w = _arrays(cost, kind)
    offs, _ = offsets(active_mask, contact_types)
    for i, o in enumerate(offs):
        if o is None:
            continue
        d = np.asarray(f[o:o + 3], dtype=float) - ref[i]
        lf[o:o + 3] += scale * w[i] * d           # evalStageCostDerivatives :98-120, evalImpactCostDerivatives :184-206
        qff[o:o + 3] += scale * w[i]              # evalStageCostHessian :123-144, evalImpactCostHessian :209-230
        if kind == "stage":                       # intermediate_stage.cpp:104-108: hf = lf / dt, h = cost / dt
            hf[o:o + 3] = w[i] * d
            h += 0.5 * float(np.sum(w[i] * d * d))
    return lf, qff, hf, h, value(f, active_mask, contact_types, cost, kind, scale)
