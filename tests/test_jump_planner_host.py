"""The host side of RTOC_GAIT_JUMP without a device: the header's value against capi.GAIT_JUMP, the two structs the jump travels in
(no member was added for it), and the Python class's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robotoc_amd import capi, planner

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rtoc_robot.h")


def _defines():
    with open(HEADER) as f:
        return {k: int(v) for k, v in re.findall(r"^#define (RTOC_\w+) (-?\d+)\b", f.read(), flags=re.M)}


def test_the_header_and_the_python_shell_agree_on_the_gaits():
    d = _defines()
    assert d["RTOC_GAIT_JUMP"] == capi.GAIT_JUMP == 5
    names = ("TROT", "CRAWL", "PACE", "FLYING_TROT", "BIPED_WALK", "JUMP")
    assert [d["RTOC_GAIT_" + n] for n in names] == [getattr(capi, "GAIT_" + n) for n in names] == list(range(6))
    assert planner.JumpFootStepPlanner.GAIT == capi.GAIT_JUMP


def test_the_structs_are_unchanged():
    # rtoc_foot_step_planner: 4 ints, 3 + 4 + 4 doubles; rtoc_foot_step_ref_params: 6 ints, 16 doubles, 4 ints, 3 doubles, 2 ints, 3 doubles, 2 ints
    assert C.sizeof(capi.FootStepPlanner) == 4 * 4 + 11 * 8 == 104
    assert C.sizeof(capi.FootStepRefs) == 6 * 4 + 16 * 8 + 4 * 4 + 3 * 8 + 2 * 4 + 3 * 8 + 2 * 4 == 232
    with open(HEADER) as f:
        text = f.read()
    body = text[text.index("typedef struct rtoc_foot_step_planner {"):text.index("} rtoc_foot_step_planner;")]
    assert len(re.findall(r"^\s+(?:int|double) ", body, flags=re.M)) == 7   # the members' lines, as before the jump


class _Ctx:
    batch, _model_ncontacts = 3, 4

    def set_foot_step_planner(self, structs):
        self.structs = structs


def test_set_jump_pattern_fills_the_structs():
    ctx = _Ctx()
    pl = planner.JumpFootStepPlanner(ctx, capi.PROJECT_YAW)
    pl.set_jump_pattern([0.5, 0.1, 0.0], 0.3)
    p = ctx.structs   # one struct for the batch
    assert isinstance(p, capi.FootStepPlanner)
    assert (p.gait, p.mode, p.projection, p.enable_stance_phase) == (capi.GAIT_JUMP, capi.FOOT_STEP_FIXED, capi.PROJECT_YAW, 0)
    assert list(p.step_length) == [0.5, 0.1, 0.0] and p.step_yaw == 0.3
    pl.set_jump_pattern(np.arange(9.0).reshape(3, 3), [0.1, 0.2, 0.3])
    assert len(ctx.structs) == 3 and list(ctx.structs[2].step_length) == [6.0, 7.0, 8.0] and ctx.structs[1].step_yaw == 0.2
    with pytest.raises(ValueError):
        pl.set_jump_pattern(np.zeros((2, 3)), 0.0)
    with pytest.raises(TypeError):
        pl.set_raibert_gait_pattern([0, 0, 0], 0.0, 0.2, 0.1, 0.7)
    with pytest.raises(TypeError):
        pl.set_gait_pattern([0, 0, 0], 0.0, False)
