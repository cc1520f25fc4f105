"""Every grid structure rtoc_set_grid accepts, enumerated: words over five kinds of non-terminal grid point, each built from
a uniform grid by setting type, dims and switching_constraint.  Shared by tests/test_grid_words.py (CPU: counts, the oracle
against the dense KKT solve, the oracle's own sensitivity) and tests/test_every_grid_gpu.py (every backward path on every word).

No sto / sto_next flags here: they only mean something as TimeDiscretization produces them (tests/test_random_grids.py)."""
import itertools

from robotoc_amd.grid import uniform_grid
from robotoc_amd.types import GRID_IMPACT, GRID_LIFT, anymal_dims, icub_dims

# R regular, C regular with a switching constraint, L lift, Lc lift with a switching constraint, I impact
KINDS = ("R", "C", "L", "Lc", "I")
DT = 0.02

# the sets of the CPU tests: robot shape, rows of every switching constraint, longest word enumerated against the dense KKT solve.
# ANYmal takes 6 rows, not dims == nu == 12: two such constraints in one horizon make the recursion itself ill conditioned.
SHAPES = {"anymal": (anymal_dims(), 6, 5), "icub32": (icub_dims(32), 6, 4), "icub35": (icub_dims(35), 12, 4)}


def valid(word):
    """rtoc_set_grid's rules on the non-terminal points (the terminal point is appended by build): no impact at index 0 or at
    nstages - 2 and beyond (nstages = len(word) + 1), no lift at index 0."""
    n = len(word) + 1
    for i, k in enumerate(word):
        if k == "I" and (i == 0 or i >= n - 2):
            return False
        if k in ("L", "Lc") and i == 0:
            return False
    return len(word) >= 1


def build(word, rows):
    """The grid of `word`: len(word) points of the given kinds and the terminal point; `rows` = rows of every switching constraint."""
    grids = uniform_grid(len(word), DT, dimf=12)
    for g, k in zip(grids, word):
        if k in ("L", "Lc"):
            g.type = GRID_LIFT
        elif k == "I":
            g.type = GRID_IMPACT
        if k in ("C", "Lc"):
            g.dims = rows
            g.switching_constraint = 1
    return grids


def words(max_len):
    """Every valid word of length 1 ... max_len, in itertools.product order."""
    out = []
    for n in range(1, max_len + 1):
        out += [w for w in itertools.product(KINDS, repeat=n) if valid(w)]
    return out


def sample(length, step):
    """Every step-th valid word of that length, in the same order (deterministic: no RNG)."""
    return [w for w in itertools.product(KINDS, repeat=length) if valid(w)][::step]


def name(word):
    return " ".join(word)
