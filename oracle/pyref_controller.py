"""TEST INFRASTRUCTURE ONLY: one robot's control period as the reference runs it, with the TrajectoryMemory that it
carries from one period to the next. PARITY UNPINNED (the reference holds no fixtures for
it); checked against the C++ host adapter and the batch statements by tests/test_controller_sequence.py.

The control flow and the memory are stated here on their own, as plain lists, with no `valid` flag and no `length`:
a record is the list the reference holds, and "empty" means a list of length 0. The arithmetic inside the stages is
shared with the other restatements (pyref_path_handler, pyref_trajectorize, pyref_format.yaw_roundtrip).

Follows, per robot:
  SocialMPCController::computeVelocityCommands     reference src/social_mpc_controller.cpp:162-257
    transformGlobalPlan throws                      src/path_handler.cpp:44-47, 100-103 -> no command, memory untouched
    trajectorize returns false                      src/social_mpc_controller.cpp:180-189 -> (0.1, 0), memory untouched
    optimize returns false                          src/social_mpc_controller.cpp:240-245 -> cmds = init_cmds
    the returned command                            src/social_mpc_controller.cpp:250-256 -> cmds[0]
  Optimizer::optimize                               reference src/optimizer.cpp:148-452
    fewer than 2 poses                              :158-162 (before the memory is seeded)
    an empty record is seeded with the uncut path   :177-183 (the cut of :492-497 happens later, on the caller's copy)
    format_to_optimize                              :484-551
    the solve inputs taken from optim_status        :204-237
    the solve is not usable                         :384-388 (before the store)
    the store                                       :448-449

This project's convention for SMPC_NOT_SOLVED (-1, a scene that a device `order` left out; the reference has no such
state): it is treated like an unusable solve. Nothing is stored, and the command is init_cmds[0].

Where the reference's behaviour is undefined, the robot is marked (`undefined` holds the reason) and a caller stops
comparing it from then on:
  * format_to_optimize reads previous_cmds[i - 1] past the end of the record (:539-544 index it without a bound: a
    path longer than the record by more than one pose);
  * optimize returns false with an empty init_cmds (a 1-pose trajectorizer path), so cmds[0] reads an empty vector.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from .pyref_format import yaw_roundtrip

CONVERGENCE, NO_CONVERGENCE, FAILURE, NOT_SOLVED = 0, 1, 2, -1
SRC_OPTIMISED, SRC_INIT_CMDS, SRC_CREEP, SRC_NONE = 0, 1, 2, 3


def usable(status) -> bool:
    """summary.IsSolutionUsable() (:384): convergence or the iteration cap. FAILURE and NOT_SOLVED are not usable."""
    return int(status) in (CONVERGENCE, NO_CONVERGENCE)


@dataclass
class Tick:
    source: int                   # SRC_*: which branch of computeVelocityCommands produced the command
    cmd: tuple = None             # (linear.x, angular.z); None for SRC_NONE or when undefined
    inputs: dict = None           # what optimize handed the solver, when it got that far
    status: int = None            # the injected solve's status, when it was called
    undefined: str = None         # set when this tick made the reference's behaviour undefined


@dataclass
class RobotController:
    """One robot. current_path_w / current_cmds_w / time_step / max_time: the reference's floats; nb: parameter blocks
    of the batch's horizon (init_params holds the first min(nb, kept) velocities, as the batch arrays lay them out)."""
    current_path_w: float
    current_cmds_w: float
    time_step: float
    max_time: float
    nb: int
    previous_path: list = field(default_factory=list)   # [(x, y, yaw)]
    previous_cmds: list = field(default_factory=list)   # [(linear.x, angular.z)]
    undefined: str = None

    def max_poses(self) -> int:
        """(int)round(maxtime / timestep) in float (:492), round half away from zero."""
        q = float(np.float32(self.max_time) / np.float32(self.time_step))
        return int(math.floor(q + 0.5))

    # -- Optimizer::format_to_optimize (:484-551) on lists ---------------------------------------------------------
    def format_to_optimize(self, path, cmds, speed):
        """path: list of (x, y, yaw), cmds: list of (v, w); returns the optim_status rows (x, y, yaw, t, lv, av), or
        None when previous_cmds would be read past its end (undefined)."""
        maxsize = self.max_poses()
        if len(path) > maxsize:                                  # :492-497, the caller's copy only
            path = path[:maxsize - 1]
        wp = float(np.float32(self.current_path_w))
        wc = float(np.float32(self.current_cmds_w))
        ts = np.float32(self.time_step)
        prev_p, prev_c = self.previous_path, self.previous_cmds
        rows = []
        for i in range(len(path)):
            x, y, yaw = path[i]
            if len(prev_p) != 0 and i < len(prev_p):             # :506
                px, py, pyaw = prev_p[i]
                x, y = wp * x + (1.0 - wp) * px, wp * y + (1.0 - wp) * py
                yaw = yaw_roundtrip(wp * path[i][2] + (1.0 - wp) * pyaw)
            t = float(np.float32(i) * ts)                        # :526, unsigned times float
            if i == 0:                                           # :530-534
                lv, av = float(speed[0]), float(speed[1])
            else:                                                # :537-547
                if i - 1 >= len(prev_c):
                    return None
                lv = wc * cmds[i - 1][0] + (1.0 - wc) * prev_c[i - 1][0]
                av = wc * cmds[i - 1][1] + (1.0 - wc) * prev_c[i - 1][1]
            rows.append((x, y, yaw, t, lv, av))
        return rows

    def solve_inputs(self, rows):
        """What optimize takes from optim_status (:204-237): the start pose through setRPY / getYaw, the path points, the
        final heading, the horizon after the pop_back, and the initial velocities of the parameter blocks."""
        kept = len(rows)
        return {"robot_status": np.array(rows, np.float64).reshape(kept, 6),
                "pose0": np.array([rows[0][0], rows[0][1], yaw_roundtrip(rows[0][2])]),
                "path_pts": np.array([(r[0], r[1]) for r in rows]),
                "goal_yaw": rows[-1][2],
                "T_scene": kept - 1,
                "init_params": np.array([v for r in rows[:min(self.nb, kept)] for v in (r[4], r[5])])}

    # -- Optimizer::optimize (:148-452) -----------------------------------------------------------------------------
    def optimize(self, path, cmds, speed, solve):
        """Returns (ok, cmds_out, inputs, status); ok is None when the reference's behaviour is undefined."""
        if len(path) < 2:                                        # :158-162, before the seed
            return False, None, None, None
        if len(self.previous_path) == 0:                         # :177-183, the whole incoming path and commands
            self.previous_path = [tuple(p) for p in path]
            self.previous_cmds = [tuple(c) for c in cmds]
        rows = self.format_to_optimize(path, cmds, speed)
        if rows is None:
            return None, None, None, None
        inputs = self.solve_inputs(rows)
        status, out_cmds, out_path = solve(inputs)
        if not usable(status):                                   # :384-388 (and this project's NOT_SOLVED)
            return False, None, inputs, int(status)
        self.previous_path = [tuple(p) for p in out_path]        # :448-449
        self.previous_cmds = [tuple(c) for c in out_cmds]
        return True, [tuple(c) for c in out_cmds], inputs, int(status)

    # -- SocialMPCController::computeVelocityCommands (src/social_mpc_controller.cpp:162-257) ------------------------
    def tick_from_trajectory(self, window_error, traj_ok, path, cmds, speed, solve) -> Tick:
        """window_error: transformGlobalPlan threw; traj_ok: trajectorize's return value; path / cmds: its output
        (n poses, n - 1 commands); solve(inputs) -> (status, cmds, path) of T_scene + 1 entries each."""
        if window_error:                                         # path_handler.cpp:44-47, 100-103
            return Tick(SRC_NONE)
        if not traj_ok:                                          # :180-189
            return Tick(SRC_CREEP, (0.1, 0.0))
        init_cmds = [tuple(c) for c in cmds]                     # :190
        ok, out_cmds, inputs, status = self.optimize(path, cmds, speed, solve)
        if ok is None:
            self.undefined = "previous_cmds read past the end of the record"
            return Tick(SRC_INIT_CMDS, None, inputs, status, self.undefined)
        if not ok:                                               # :241-245
            if len(init_cmds) == 0:
                self.undefined = "optimize failed on a path without commands: cmds[0] of an empty vector"
                return Tick(SRC_INIT_CMDS, None, inputs, status, self.undefined)
            return Tick(SRC_INIT_CMDS, init_cmds[0], inputs, status)
        return Tick(SRC_OPTIMISED, out_cmds[0], inputs, status)  # :250-256

    def tick(self, plan, start, robot_pose, speed, solve, traj_params, window):
        """The whole period from the global plan: transformGlobalPlan (pyref_path_handler) with window = (search
        distance, threshold), then trajectorize (pyref_trajectorize) on the window. Returns (Tick, new plan start)."""
        from . import pyref_path_handler, pyref_trajectorize
        win, new_start, werr = pyref_path_handler.transform_global_plan(plan, start, robot_pose, window[0], window[1])
        if werr:
            return self.tick_from_trajectory(True, False, [], [], speed, solve), new_start
        tp = traj_params
        p, c, terr = pyref_trajectorize.trajectorize(win, robot_pose, tp.omnidirectional, tp.desired_linear_vel,
                                                     tp.lookahead_dist, tp.max_angular_vel, tp.time_step, tp.max_time)
        if p is None:
            return self.tick_from_trajectory(False, False, [], [], speed, solve), new_start
        path = [tuple(r) for r in p]
        cmds = [(r[0], r[2]) for r in c]
        return self.tick_from_trajectory(False, True, path, cmds, speed, solve), new_start
