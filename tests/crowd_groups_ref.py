"""CPU checker of smpc_crowd_step_groups_batch, written from the contract in include/smpc.h: tests/crowd_ref.py's plain
per-person loop (its social term, obstacle lookup, heading and wrap are imported, not copied) with the group force of
sfm.hpp computeGroupForce added after the obstacle force, by math.acos and math.tanh. TEST INFRASTRUCTURE ONLY.

step() advances one robot's persons, step_batch() a batch; both return new arrays and leave their inputs alone. A person
without a group force takes exactly the arithmetic of crowd_ref.step (the addition is skipped, not made with zero).
margins() reports how far one robot's grouped persons stay from the decisions the group force takes."""
import math

import numpy as np

import crowd_ref as R

GAZE, COHERENCE, REPULSION = 3.0, 2.0, 1.0   # sfm.hpp forceFactorGroupGaze / GroupCoherence / GroupRepulsion
FACTORS = (GAZE, COHERENCE, REPULSION)


def members_of(i, count, group_id):
    """rows of person i's group (i included), or [] when i has no group id"""
    if group_id is None or int(group_id[i]) < 0:
        return []
    return [j for j in range(int(count)) if int(group_id[j]) == int(group_id[i])]


def desired_direction(px, py, has_goal, goal, goal_radius):
    """what computeDesiredForce returns as the desired direction; (0, 0) where the reference leaves it uninitialised"""
    if has_goal:
        d = math.sqrt((goal[0] - px) ** 2 + (goal[1] - py) ** 2)
        if d > goal_radius:
            return (goal[0] - px) / d, (goal[1] - py) / d
    return 0.0, 0.0


def gaze_terms(px, py, dd, centre, size):
    """(e, |dd|, |rel|, rel) of the gaze force: rel = the others' centre of mass seen from the person"""
    cx, cy = (size * centre[0] - px) / (size - 1), (size * centre[1] - py) / (size - 1)
    rel = (cx - px, cy - py)
    return dd[0] * rel[0] + dd[1] * rel[1], math.hypot(*dd), math.hypot(*rel), rel


def group_force(i, old, count, group_id, dd, person_radius, factors=FACTORS):
    """The group force on person i, or None when there is none (no id, or fewer than two members)."""
    mem = members_of(i, count, group_id)
    size = len(mem)
    if size < 2:
        return None
    px, py = float(old[i, 0]), float(old[i, 1])
    centre = (sum(float(old[j, 0]) for j in mem) / size, sum(float(old[j, 1]) for j in mem) / size)
    fx = fy = 0.0
    # gaze
    e, ndd, nrel, _ = gaze_terms(px, py, dd, centre, size)
    if ndd > 0.0 and nrel > 0.0:
        c = e / (ndd * nrel)
        if math.isfinite(c) and math.acos(min(1.0, max(-1.0, c))) > math.pi / 2:
            fx += factors[0] * (e / (ndd * ndd)) * dd[0]
            fy += factors[0] * (e / (ndd * ndd)) * dd[1]
    # coherence
    rx, ry = centre[0] - px, centre[1] - py
    soft = (math.tanh(math.hypot(rx, ry) - (size - 1) / 2.0) + 1.0) / 2.0
    fx += rx * factors[1] * soft
    fy += ry * factors[1] * soft
    # repulsion
    sx = sy = 0.0
    for j in mem:
        if j != i:
            ux, uy = px - float(old[j, 0]), py - float(old[j, 1])
            if math.hypot(ux, uy) < 2.0 * person_radius:
                sx, sy = sx + ux, sy + uy
    return fx + factors[2] * sx, fy + factors[2] * sy


def step(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, goal_radius=0.25, person_radius=0.35,
         desired_speed=0.6, cyclic=True, robot_visible=True, desired_speeds=None, od_indexes=None, od_origin=None,
         od_resolution=None, events=None, group_id=None, factors=FACTORS, forces=None):
    """crowd_ref.step with group_id [Np] (None: no groups) and factors (gaze, coherence, repulsion).
    forces: a list that receives every person's total force (fx, fy)."""
    people, cursor = np.array(people, np.float64), np.array(cursor, np.int32)
    old = people.copy()
    K = waypoints.shape[1]
    rvx, rvy = twist[0] * math.cos(pose[2]), twist[0] * math.sin(pose[2])
    for i in range(int(count)):
        px, py, vx, vy = (float(v) for v in old[i, 0:4])
        des = float(desired_speed if desired_speeds is None else desired_speeds[i])
        nwp = min(max(int(n_waypoints[i]), 0), K)
        cur = int(cursor[i])
        has_goal = 0 <= cur < nwp
        fx, fy = -vx / R.RELAX, -vy / R.RELAX
        gx = gy = 0.0
        if has_goal:
            gx, gy = (float(v) for v in waypoints[i, cur])
            d = math.sqrt((gx - px) ** 2 + (gy - py) ** 2)
            if d > goal_radius:
                fx = R.F_DESIRED * ((gx - px) / d * des - vx) / R.RELAX
                fy = R.F_DESIRED * ((gy - py) / d * des - vy) / R.RELAX
        if robot_visible:
            sx, sy = R.social_term(pose[0] - px, pose[1] - py, vx - rvx, vy - rvy)
            fx, fy = fx + sx, fy + sy
        for j in range(int(count)):
            if j != i:
                sx, sy = R.social_term(old[j, 0] - px, old[j, 1] - py, vx - old[j, 2], vy - old[j, 3])
                fx, fy = fx + sx, fy + sy
        o = R.obstacle_of(px, py, od_indexes, od_origin, od_resolution)
        if o is not None:
            mx, my = px - o[0], py - o[1]
            m = math.sqrt(mx * mx + my * my)
            e = R.F_OBSTACLE * math.exp(-(m - person_radius) / R.SIGMA)
            if m > 0.0:
                fx, fy = fx + e * mx / m, fy + e * my / m
        grp = group_force(i, old, count, group_id, desired_direction(px, py, has_goal, (gx, gy), goal_radius), person_radius, factors)
        if grp is not None:
            fx, fy = fx + grp[0], fy + grp[1]
        if forces is not None:
            forces.append((fx, fy))
        nvx, nvy = vx + fx * dt, vy + fy * dt
        sp = math.sqrt(nvx * nvx + nvy * nvy)
        if sp > des:
            nvx, nvy = nvx / sp * des, nvy / sp * des
        vz = R.wrap(R.heading(nvx, nvy) - R.heading(vx, vy)) / dt
        px, py = px + nvx * dt, py + nvy * dt
        if has_goal and math.sqrt((gx - px) ** 2 + (gy - py) ** 2) <= goal_radius:
            cur += 1
            if events is not None:
                events["arrived"] = events.get("arrived", 0) + 1
                if cyclic and cur >= nwp:
                    events["wrapped"] = events.get("wrapped", 0) + 1
        if cyclic and cur >= nwp:
            cur = 0
        people[i] = [px, py, nvx, nvy, vz]
        cursor[i] = cur
    return people, cursor


def step_batch(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, desired_speeds=None, od_indexes=None,
               od_origin=None, od_resolution=None, events=None, group_id=None, **kw):
    """Batch of robots; group_id [B,Np] or None; the grids as in crowd_ref.step_batch."""
    people, cursor = np.array(people, np.float64), np.array(cursor, np.int32)
    shared = od_indexes is not None and np.ndim(od_indexes) == 2
    for b in range(people.shape[0]):
        idx = None if od_indexes is None else (od_indexes if shared else od_indexes[b])
        org = None if od_indexes is None else (np.reshape(od_origin, (-1, 2))[0] if shared else od_origin[b])
        people[b], cursor[b] = step(dt, people[b], cursor[b], pose[b], twist[b], count[b], waypoints[b], n_waypoints[b],
                                    desired_speeds=None if desired_speeds is None else desired_speeds[b], od_indexes=idx,
                                    od_origin=org, od_resolution=od_resolution, events=events,
                                    group_id=None if group_id is None else group_id[b], **kw)
    return people, cursor


def margins(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, group_id=None, goal_radius=0.25,
            person_radius=0.35, **kw):
    """The least distances of one robot's grouped persons (groups of two or more) from the group force's decisions:
    gaze (|e| / (|dd| |rel|), the cosine of the gaze angle, from 0; persons with a desired direction only), reach (of the
    distance between two members from 2 * person_radius), rel (|rel| of the gaze term from 0, where a gaze term exists),
    goal (of every person's distance to its goal after the step WITH the group force from goal_radius), grouped (how many
    persons have a group force)."""
    new, _ = step(dt, people, cursor, pose, twist, count, waypoints, n_waypoints, group_id=group_id, goal_radius=goal_radius,
                  person_radius=person_radius, **kw)
    m = dict(gaze=math.inf, reach=math.inf, rel=math.inf, goal=math.inf, grouped=0)
    K = waypoints.shape[1]
    for i in range(int(count)):
        cur = int(cursor[i])
        has_goal = 0 <= cur < min(max(int(n_waypoints[i]), 0), K)
        if has_goal:
            g = waypoints[i, cur]
            m["goal"] = min(m["goal"], abs(math.hypot(g[0] - new[i, 0], g[1] - new[i, 1]) - goal_radius))
        mem = members_of(i, count, group_id)
        if len(mem) < 2:
            continue
        m["grouped"] += 1
        px, py = float(people[i, 0]), float(people[i, 1])
        for j in mem:
            if j != i:
                m["reach"] = min(m["reach"], abs(math.hypot(px - people[j, 0], py - people[j, 1]) - 2.0 * person_radius))
        dd = desired_direction(px, py, has_goal, waypoints[i, cur] if has_goal else (0.0, 0.0), goal_radius)
        if dd != (0.0, 0.0):
            size = len(mem)
            centre = (sum(float(people[j, 0]) for j in mem) / size, sum(float(people[j, 1]) for j in mem) / size)
            e, ndd, nrel, _ = gaze_terms(px, py, dd, centre, size)
            m["rel"] = min(m["rel"], nrel)
            if nrel > 0.0:
                m["gaze"] = min(m["gaze"], abs(e) / (ndd * nrel))
    return m
