"""Host-side mirror of the reference's `OptimizerParams` (optimizer.hpp:59-101, src/optimizer.cpp:16-85).

Field names follow the reference's ROS parameter names (`<plugin>.optimizer.*`, `<plugin>.optimizer.weights.*`,
`<plugin>.trajectorizer.{time_step,max_time}`); defaults are the reference's *code* defaults. `from_yaml`
reads a params/*.yaml-shaped file (the `FollowPath:` section of a Nav2 controller_server configuration).
"""
from dataclasses import dataclass, asdict, fields

import numpy as np

from ._abi import LINEAR_SOLVER, SCENE_PARAM_FIELDS, SmpcParams

# the OptimizerParams field behind each smpc_scene_params field (struct order)
SCENE_ROW_FIELDS = ("distance_weight", "social_weight", "velocity_weight", "angle_weight", "agent_angle_weight",
                    "proxemics_weight", "velocity_feasibility_weight", "obstacle_weight", "goal_align_weight",
                    "desired_linear_vel", "v_min", "v_max", "w_min", "w_max")
assert len(SCENE_ROW_FIELDS) == len(SCENE_PARAM_FIELDS)


@dataclass
class TrajectorizerParams:
    """`<plugin>.trajectorizer.*` of PathTrajectorizer::configure (src/path_trajectorizer.cpp:53-84), code defaults."""
    omnidirectional: bool = False
    desired_linear_vel: float = 0.4
    lookahead_dist: float = 0.4
    max_angular_vel: float = 1.0
    time_step: float = 0.05
    max_time: float = 3.0

    @property
    def max_steps(self) -> int:
        """(int)round(max_time / time_step), doubles (src/path_trajectorizer.cpp:84)."""
        return int(np.round(self.max_time / self.time_step))


@dataclass
class MetricsParams:
    """What smpc_episode_metrics_batch compares a sample with (smpc_metrics_batch, include/smpc.h): the goal tolerance, the
    robot's and a person's radius (a collision with a person: centres closer than their sum; with an obstacle: clearance
    below the robot's), and the proxemic zones around a person's centre (Hall's intimate / personal / social distances)."""
    goal_tolerance: float = 0.25
    robot_radius: float = 0.3
    person_radius: float = 0.3
    intimate_radius: float = 0.45
    personal_radius: float = 1.2
    social_radius: float = 3.6

    def __post_init__(self):
        for f in fields(self):
            if not getattr(self, f.name) >= 0.0:
                raise ValueError(f"MetricsParams.{f.name} must be >= 0, got {getattr(self, f.name)}")


@dataclass
class CrowdParams:
    """The reactive crowd of a closed-loop episode (smpc_crowd_batch, include/smpc.h): the Social Force Model step that
    moves every robot's persons each control period. goal_radius: a waypoint counts as reached within it; person_radius:
    a person's body in the obstacle force (sfm.hpp Agent default); desired_speed: of every person without a speed of its
    own; cyclic: a person that reached its last waypoint heads for the first one again (sfm.hpp cyclicGoals), otherwise it
    comes to rest there; robot_visible: the persons give way to the robot as they do to each other."""
    goal_radius: float = 0.25
    person_radius: float = 0.35
    desired_speed: float = 0.6
    cyclic: bool = True
    robot_visible: bool = True

    def __post_init__(self):
        if not self.goal_radius >= 0.0 or not self.person_radius >= 0.0:
            raise ValueError(f"CrowdParams radii must be >= 0, got {self.goal_radius}, {self.person_radius}")
        if not self.desired_speed > 0.0:
            raise ValueError(f"CrowdParams.desired_speed must be > 0, got {self.desired_speed}")


@dataclass
class PoolCrowdParams:
    """The reactive crowd of a shared world (smpc_crowd_pool_in, include/smpc_crowd_pool.h; BatchEpisode(pool_crowd=...)):
    the Social Force Model step that moves the shared pedestrians each control period. interaction_range: a pedestrian gives
    way to every agent of the table (pedestrians and robots) within it, in metres; the other fields as CrowdParams."""
    interaction_range: float = 5.0
    goal_radius: float = 0.25
    person_radius: float = 0.35
    desired_speed: float = 0.6
    cyclic: bool = True

    def __post_init__(self):
        if not (np.isfinite(self.interaction_range) and self.interaction_range > 0.0):
            raise ValueError(f"PoolCrowdParams.interaction_range must be finite and > 0, got {self.interaction_range}")
        if not self.goal_radius >= 0.0 or not self.person_radius >= 0.0:
            raise ValueError(f"PoolCrowdParams radii must be >= 0, got {self.goal_radius}, {self.person_radius}")
        if not self.desired_speed > 0.0:
            raise ValueError(f"PoolCrowdParams.desired_speed must be > 0, got {self.desired_speed}")


@dataclass
class CrowdGroupParams:
    """The group force of the reactive crowd (smpc_crowd_groups, include/smpc.h; sfm.hpp forceFactorGroupGaze /
    GroupCoherence / GroupRepulsion): companions look towards each other, stay together and do not overlap."""
    factor_gaze: float = 3.0
    factor_coherence: float = 2.0
    factor_repulsion: float = 1.0

    def __post_init__(self):
        for f in fields(self):
            v = getattr(self, f.name)
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"CrowdGroupParams.{f.name} must be finite and >= 0, got {v}")


@dataclass
class PlanSmootherParams:
    """Plan smoothing (include/smpc_plan_smoother.h; GlobalPlanParams(smoother=...)): wherever the planner has walked the plans,
    their inner rows are relaxed towards the mean of their neighbours (w_smooth) while a data term holds them to the rows the
    round started from (w_data), in Jacobi sweeps that never move a row into an impassable cell. A round ends at the first
    sweep that moves no row by more than `tolerance` metres, or after max_its sweeps; refinement_num further rounds start
    from the rows the round before ended with. The defaults are those of Nav2's simple smoother, as recalled.
    lethal_min_cost / allow_unknown: which cells are passable; None: the planner's values."""
    w_data: float = 0.2
    w_smooth: float = 0.3
    tolerance: float = 1e-10
    max_its: int = 1000
    refinement_num: int = 2
    lethal_min_cost: int = None
    allow_unknown: bool = None

    MAX_POSES, MAX_ITS, MAX_REFINEMENTS = 1024, 100000, 8   # include/smpc_plan_smoother.h's limits

    def __post_init__(self):
        if not (np.isfinite(self.w_data) and self.w_data > 0.0):
            raise ValueError(f"PlanSmootherParams.w_data must be finite and > 0, got {self.w_data}")
        if not (np.isfinite(self.w_smooth) and self.w_smooth >= 0.0):
            raise ValueError(f"PlanSmootherParams.w_smooth must be finite and >= 0, got {self.w_smooth}")
        if not np.float64(self.w_data) + np.float64(4.0) * np.float64(self.w_smooth) < 2.0:
            raise ValueError("PlanSmootherParams: w_data + 4 * w_smooth must be < 2 (the sweep would not contract)")
        if not self.tolerance >= 0.0:
            raise ValueError(f"PlanSmootherParams.tolerance must be >= 0, got {self.tolerance}")
        if int(self.max_its) != self.max_its or self.max_its < 1:
            raise ValueError(f"PlanSmootherParams.max_its must be an integer >= 1, got {self.max_its}")
        if int(self.refinement_num) != self.refinement_num or self.refinement_num < 0:
            raise ValueError(f"PlanSmootherParams.refinement_num must be an integer >= 0, got {self.refinement_num}")
        if self.lethal_min_cost is not None and not 0 <= self.lethal_min_cost <= 255:
            raise ValueError(f"PlanSmootherParams.lethal_min_cost must be 0..255 or None, got {self.lethal_min_cost}")

    def supported(self, max_poses: int) -> bool:
        """Does the library smooth plans of max_poses rows with these parameters (include/smpc_plan_smoother.h's
        SMPC_ERR_UNSUPPORTED, the world's size apart)?"""
        return int(max_poses) <= self.MAX_POSES and self.max_its <= self.MAX_ITS and self.refinement_num <= self.MAX_REFINEMENTS


@dataclass
class GlobalPlanParams:
    """Global plans on a world map (include/smpc_global_plan.h): what entering a cell costs, w = neutral_cost + cost_weight *
    cost (integers: a goal field is exact), which cells are passable (cost < lethal_min_cost, and 255 with allow_unknown),
    the rows of a plan (max_poses) and how many path cells lie between two poses (stride). smoother: the plans are smoothed
    wherever they are walked (PlanSmootherParams; None: they are handed on as walked)."""
    neutral_cost: int = 50
    cost_weight: int = 1
    lethal_min_cost: int = 253
    allow_unknown: bool = False
    max_poses: int = 400
    stride: int = 1
    smoother: PlanSmootherParams = None

    def __post_init__(self):
        if self.smoother is not None and not isinstance(self.smoother, PlanSmootherParams):
            raise ValueError("GlobalPlanParams.smoother must be a PlanSmootherParams or None")
        if self.neutral_cost < 1 or self.cost_weight < 0 or self.neutral_cost + 255 * self.cost_weight > 65535:
            raise ValueError("GlobalPlanParams: neutral_cost >= 1, cost_weight >= 0 and neutral_cost + 255 * cost_weight <= 65535")
        if not 0 <= self.lethal_min_cost <= 255:
            raise ValueError(f"GlobalPlanParams.lethal_min_cost must be 0..255, got {self.lethal_min_cost}")
        if self.max_poses < 2 or self.stride < 1:
            raise ValueError("GlobalPlanParams: max_poses >= 2 and stride >= 1")

    def world_supported(self, cells_x: int, cells_y: int) -> bool:
        """Does the library take a world of this size with these costs (include/smpc_global_plan.h's two
        SMPC_ERR_UNSUPPORTED)? Potentials are 32 bits: no path may cost 2^32 - 1 (the marker of an unreachable cell) or more."""
        cells = int(cells_x) * int(cells_y)
        return cells < 2 ** 31 and cells * 7 * (self.neutral_cost + 255 * self.cost_weight) < 2 ** 32 - 1


@dataclass
class VisibilityParams:
    """The line-of-sight filter of the people a robot perceives on a world map (include/smpc_visibility.h): the detector's
    range in metres, which cells block sight (cost >= occlusion_min_cost, and 255 only with unknown_occludes)."""
    max_range: float = 10.0
    occlusion_min_cost: int = 254
    unknown_occludes: bool = False

    def __post_init__(self):
        if not (np.isfinite(self.max_range) and self.max_range > 0.0):
            raise ValueError(f"VisibilityParams.max_range must be finite and > 0, got {self.max_range}")
        if not 0 <= self.occlusion_min_cost <= 255:
            raise ValueError(f"VisibilityParams.occlusion_min_cost must be 0..255, got {self.occlusion_min_cost}")

    def supported(self, resolution: float) -> bool:
        """Does the library take this range on a map of this resolution (include/smpc_visibility.h's SMPC_ERR_UNSUPPORTED)?
        A ray may span at most 32768 cells: max_range / resolution <= 32768, the quotient of the two doubles."""
        return bool(np.float64(self.max_range) / np.float64(resolution) <= 32768.0)


@dataclass
class SensorParams:
    """Sensed local costmaps (include/smpc_sensed_costmap.h; BatchEpisode(sensor=...)): every tick one 360-degree scan of
    n_beams beams out to max_range metres marks the cells it stops at (world cells with cost >= occlusion_min_cost, 255 only
    with unknown_occludes, and the discs of agent_radius metres around the agents), and the marks are inflated as Nav2's
    InflationLayer does (inflation_radius, cost_scaling_factor, inscribed_radius). The defaults are the local costmap of the
    reference's shipped parameter files: marking out to 2.5 m, inflation radius 0.7 m, scaling 3.0. base: "free" (the
    reference's: no static layer) or "world" (the larger of the sensed cost and the world cut)."""
    n_beams: int = 360
    max_range: float = 2.5
    agent_radius: float = 0.3
    inflation_radius: float = 0.7
    cost_scaling_factor: float = 3.0
    inscribed_radius: float = 0.0
    occlusion_min_cost: int = 254
    unknown_occludes: bool = False
    base: str = "free"

    BASES = ("free", "world")

    def __post_init__(self):
        if not 1 <= int(self.n_beams) <= 4096:
            raise ValueError(f"SensorParams.n_beams must be 1..4096, got {self.n_beams}")
        for name in ("max_range", "cost_scaling_factor"):
            v = getattr(self, name)
            if not (np.isfinite(v) and v > 0.0):
                raise ValueError(f"SensorParams.{name} must be finite and > 0, got {v}")
        for name in ("agent_radius", "inflation_radius", "inscribed_radius"):
            v = getattr(self, name)
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"SensorParams.{name} must be finite and >= 0, got {v}")
        if not 0 <= self.occlusion_min_cost <= 255:
            raise ValueError(f"SensorParams.occlusion_min_cost must be 0..255, got {self.occlusion_min_cost}")
        if self.base not in self.BASES:
            raise ValueError(f"SensorParams.base must be one of {self.BASES}, got {self.base!r}")

    def beam_cells(self, resolution: float) -> np.ndarray:
        """[n_beams,2] int32: the end-cell offset of beam k is (rint(R cos t), rint(R sin t)) with t = 2 pi k / n_beams and
        R = max_range / resolution, the range in cells."""
        R = np.float64(self.max_range) / np.float64(resolution)
        t = 2.0 * np.pi * np.arange(int(self.n_beams), dtype=np.float64) / np.float64(self.n_beams)
        return np.stack([np.rint(R * np.cos(t)), np.rint(R * np.sin(t))], axis=1).astype(np.int32)

    def agent_d2(self, resolution: float) -> int:
        """An agent occupies the cells within agent_radius of its own: the squared radius in cells, rounded down."""
        ra = np.float64(self.agent_radius) / np.float64(resolution)
        return int(np.floor(ra * ra + 1e-9))

    def inflation_table(self, resolution: float):
        """(inflation_cost [d2_max + 1] uint8, d2_max): Nav2's InflationLayer::computeCost by squared cell distance: 254 at
        distance 0, 253 within inscribed_radius, else uint8(252 * exp(-cost_scaling_factor * (d - inscribed_radius))) with d
        in metres; out to r = floor(inflation_radius / resolution + 1e-9) cells, d2_max = r * r."""
        r = int(np.floor(np.float64(self.inflation_radius) / np.float64(resolution) + 1e-9))
        d2 = np.arange(r * r + 1, dtype=np.float64)
        d = np.sqrt(d2) * np.float64(resolution)
        cost = np.floor(252.0 * np.exp(-np.float64(self.cost_scaling_factor) * (d - np.float64(self.inscribed_radius))))
        cost = np.where(d <= self.inscribed_radius, 253.0, np.minimum(cost, 252.0))
        cost[0] = 254.0
        return cost.astype(np.uint8), r * r

    def supported(self, resolution: float) -> bool:
        """Does the library take these on a map of this resolution (include/smpc_sensed_costmap.h's limits)? Every beam
        within 127 cells per axis (the kernel gives longer ones the kind INVALID), an inflation radius of at most 32 cells
        and an agent_d2 below 2^31."""
        r = np.floor(np.float64(self.inflation_radius) / np.float64(resolution) + 1e-9)
        ra = np.float64(self.agent_radius) / np.float64(resolution)
        return bool(np.float64(self.max_range) / np.float64(resolution) <= 127.0 and r <= 32 and ra * ra + 1e-9 < 2.0 ** 31)


@dataclass
class ObstacleMemoryParams:
    """Sensed local costmaps with memory (include/smpc_obstacle_memory.h; BatchEpisode(sensor=..., sensor_memory=...)): a
    mark stays in the window until a later beam passes through its cell, as in Nav2's ObstacleLayer. The beams reach out to
    raytrace_range metres and clear what they pass; a hit is marked only within the sensor's max_range (Nav2's
    obstacle_max_range); the cells within footprint_radius of the robot's are cleared after marking (None: none). The
    defaults are the reference's shipped local costmap: raytrace_max_range 3.0 m and the inscribed radius of its 0.48 m
    square footprint."""
    raytrace_range: float = 3.0
    footprint_radius: float = 0.24

    def __post_init__(self):
        if not (np.isfinite(self.raytrace_range) and self.raytrace_range > 0.0):
            raise ValueError(f"ObstacleMemoryParams.raytrace_range must be finite and > 0, got {self.raytrace_range}")
        if self.footprint_radius is not None and not (np.isfinite(self.footprint_radius) and self.footprint_radius >= 0.0):
            raise ValueError(f"ObstacleMemoryParams.footprint_radius must be None or finite and >= 0, got {self.footprint_radius}")

    def check(self, sensor: "SensorParams"):
        """raytrace_range >= sensor.max_range > 0: a ray clears at least as far as it marks."""
        if not (np.isfinite(sensor.max_range) and sensor.max_range > 0.0 and self.raytrace_range >= sensor.max_range):
            raise ValueError(f"ObstacleMemoryParams.raytrace_range ({self.raytrace_range}) must be >= SensorParams.max_range "
                             f"({sensor.max_range}) > 0")

    def beam_cells(self, sensor: "SensorParams", resolution: float) -> np.ndarray:
        """[n_beams,2] int32: the sensor's beam directions (SensorParams.beam_cells) at raytrace_range."""
        self.check(sensor)
        R = np.float64(self.raytrace_range) / np.float64(resolution)
        t = 2.0 * np.pi * np.arange(int(sensor.n_beams), dtype=np.float64) / np.float64(sensor.n_beams)
        return np.stack([np.rint(R * np.cos(t)), np.rint(R * np.sin(t))], axis=1).astype(np.int32)

    @staticmethod
    def _d2(radius: float, resolution: float) -> int:
        r = np.float64(radius) / np.float64(resolution)   # SensorParams.agent_d2's rounding
        return int(np.floor(r * r + 1e-9))

    def mark_d2(self, sensor: "SensorParams", resolution: float) -> int:
        """A hit is marked within the sensor's max_range: the squared range in cells, rounded down."""
        self.check(sensor)
        return self._d2(sensor.max_range, resolution)

    def footprint_d2(self, resolution: float) -> int:
        """The squared footprint radius in cells, rounded down; -1 without a footprint."""
        return -1 if self.footprint_radius is None else self._d2(self.footprint_radius, resolution)

    def supported(self, sensor: "SensorParams", resolution: float) -> bool:
        """Does the library cast these beams (include/smpc_sensed_costmap.h's reach of 127 cells per axis), with squared
        radii that fit the struct's int32 fields?"""
        fr = 0.0 if self.footprint_radius is None else np.float64(self.footprint_radius) / np.float64(resolution)
        mr = np.float64(sensor.max_range) / np.float64(resolution)
        return bool(np.float64(self.raytrace_range) / np.float64(resolution) <= 127.0 and fr * fr + 1e-9 < 2.0 ** 31
                    and mr * mr + 1e-9 < 2.0 ** 31)


@dataclass
class TrackerParams:
    """People tracks (include/smpc_tracker.h; BatchEpisode(tracker=...)): every tick the detections are associated with
    the robot's tracks by position alone (greedy by distance inside `gate` metres of the predicted position), a matched
    track takes an alpha-beta update (position xp + alpha * r, velocity v + beta / dt * r), an unmatched one coasts with its
    velocity for at most max_missed ticks, and a new track is handed on once it has confirm_hits detections. slots: tracks
    per robot (at most 64). The defaults follow a detection every 0.1 s of a pedestrian at walking speed: a gate of 0.6 m is
    five times the step of 1.2 m/s, and 20 coasted ticks are 2 s behind a pillar."""
    alpha: float = 0.5
    beta: float = 0.2
    gate: float = 0.6
    confirm_hits: int = 3
    max_missed: int = 20
    slots: int = 16

    def __post_init__(self):
        for name in ("alpha", "beta"):
            v = getattr(self, name)
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"TrackerParams.{name} must be finite and >= 0, got {v}")
        if not (np.isfinite(self.gate) and self.gate > 0.0):
            raise ValueError(f"TrackerParams.gate must be finite and > 0, got {self.gate}")
        if int(self.confirm_hits) != self.confirm_hits or self.confirm_hits < 1:
            raise ValueError(f"TrackerParams.confirm_hits must be an integer >= 1, got {self.confirm_hits}")
        if int(self.max_missed) != self.max_missed or self.max_missed < 0:
            raise ValueError(f"TrackerParams.max_missed must be an integer >= 0, got {self.max_missed}")
        if int(self.slots) != self.slots or self.slots < 1:
            raise ValueError(f"TrackerParams.slots must be an integer >= 1, got {self.slots}")

    def gain(self, dt: float) -> float:
        """beta / dt: the velocity gain the call takes (one division, here and not in the kernel)."""
        if not (np.isfinite(dt) and dt > 0.0):
            raise ValueError(f"TrackerParams.gain: dt must be finite and > 0, got {dt}")
        return float(np.float64(self.beta) / np.float64(dt))

    def supported(self, dt: float = None) -> bool:
        """Does the library run these tracks: at most 64 slots, counters that fit the struct's int32 fields and, with `dt`, a
        finite gain?"""
        ok = self.slots <= 64 and self.confirm_hits < 2 ** 31 and self.max_missed < 2 ** 31
        with np.errstate(over="ignore"):
            return bool(ok and (dt is None or (np.isfinite(dt) and dt > 0.0 and np.isfinite(np.float64(self.beta) / np.float64(dt)))))


@dataclass
class DetectorParams:
    """People detections (include/smpc_detector.h; BatchEpisode(detector=...)): every tick the persons a robot is handed
    become what a detector would report of them. A person whose sight line passes within body_radius metres of another
    person's centre is hidden (0: no body occlusion); a visible person is missed with probability p_miss; a detected one is
    reported with a position noise of standard deviation sigma + sigma_growth * range^2 metres per axis (the sum of four
    uniform words, so bounded by 2 sqrt(3) standard deviations); each of clutter_candidates (at most 64) false detections
    exists with probability p_clutter, uniform in a square of half-side clutter_range metres around the robot. seed: the
    64-bit key of the counter-based generator; a robot's draws depend on (seed, its stream id, its tick counter, the row)
    alone. The defaults follow a leg or torso detector on a planar scan: 3 cm at the sensor, 23 cm at 10 m."""
    body_radius: float = 0.25
    p_miss: float = 0.1
    sigma: float = 0.03
    sigma_growth: float = 0.002
    clutter_candidates: int = 2
    p_clutter: float = 0.05
    clutter_range: float = 5.0
    seed: int = 0

    def __post_init__(self):
        for name in ("body_radius", "sigma", "sigma_growth", "clutter_range"):
            v = getattr(self, name)
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"DetectorParams.{name} must be finite and >= 0, got {v}")
        for name in ("p_miss", "p_clutter"):
            v = getattr(self, name)
            if not (np.isfinite(v) and 0.0 <= v <= 1.0):
                raise ValueError(f"DetectorParams.{name} must lie in [0, 1], got {v}")
        if int(self.clutter_candidates) != self.clutter_candidates or self.clutter_candidates < 0:
            raise ValueError(f"DetectorParams.clutter_candidates must be an integer >= 0, got {self.clutter_candidates}")
        if int(self.seed) != self.seed or not 0 <= self.seed < 2 ** 64:
            raise ValueError(f"DetectorParams.seed must be an integer in 0 .. 2^64 - 1, got {self.seed}")

    @staticmethod
    def _threshold(p: float) -> int:
        return min(int(np.floor(np.float64(p) * np.float64(2.0 ** 32) + np.float64(0.5))), 2 ** 32 - 1)

    def thresholds(self):
        """(miss_threshold, clutter_threshold): p * 2^32 rounded to nearest (a half upwards), clamped to 2^32 - 1; a draw
        below the threshold fires, so p = 1 misses all but one draw in 2^32."""
        return self._threshold(self.p_miss), self._threshold(self.p_clutter)

    def scales(self):
        """(noise_scale, noise_growth, clutter_scale) as the call takes them: sigma * sqrt(3) / 2^32 (the noise sum has the
        standard deviation 2^32 / sqrt(3) to within 2^-65), sigma_growth * sqrt(3) / 2^32, clutter_range / 2^31."""
        root3, two32 = np.sqrt(np.float64(3.0)), np.float64(2.0 ** 32)
        return (float(np.float64(self.sigma) * root3 / two32), float(np.float64(self.sigma_growth) * root3 / two32),
                float(np.float64(self.clutter_range) / np.float64(2.0 ** 31)))

    def key(self):
        """(seed_lo, seed_hi)"""
        return int(self.seed) & 0xFFFFFFFF, int(self.seed) >> 32

    def supported(self) -> bool:
        """Does the library run this detector: at most 64 clutter candidates?"""
        return self.clutter_candidates <= 64


@dataclass
class ScanDetectorParams:
    """People detections from the scan (include/smpc_scan_people.h; BatchEpisode(sensor=..., scan_detector=...)): every tick
    the cells the scan's beams stopped at are clustered into segments, and a segment of a person's size is a detection.
    Neighbouring hits within link_distance metres are linked; a segment needs at least min_points beams and a distance
    between its first and last hit of min_width .. max_width metres; the centre of its cells is pushed body_offset metres
    away from the robot, since the visible arc lies in front of the body's centre. subtract_map: hits on occluding cells of
    the world map are background (a deployment's static-map subtraction); without it a pillar of a person's width is a
    detection. max_range: hits beyond it are background; None: the sensor's marking range (SensorParams.max_range, also
    under sensor_memory, whose beams reach further). max_detections: rows per robot (at most 64). All lengths become
    squared cell distances rounded down, as SensorParams.agent_d2 rounds. The defaults suit discs of 0.3 m on cells of
    0.05 m seen by 360 beams: from a link distance of 0.2 m on a lone person is one segment."""
    link_distance: float = 0.25
    min_points: int = 3
    min_width: float = 0.2
    max_width: float = 0.8
    body_offset: float = 0.2
    subtract_map: bool = True
    max_range: float = None
    max_detections: int = 16

    def __post_init__(self):
        for name in ("link_distance", "min_width", "max_width", "body_offset"):
            v = getattr(self, name)
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"ScanDetectorParams.{name} must be finite and >= 0, got {v}")
        if self.min_width > self.max_width:
            raise ValueError(f"ScanDetectorParams.min_width ({self.min_width}) must be <= max_width ({self.max_width})")
        if self.max_range is not None and not (np.isfinite(self.max_range) and self.max_range > 0.0):
            raise ValueError(f"ScanDetectorParams.max_range must be None or finite and > 0, got {self.max_range}")
        if int(self.min_points) != self.min_points or self.min_points < 1:
            raise ValueError(f"ScanDetectorParams.min_points must be an integer >= 1, got {self.min_points}")
        if int(self.max_detections) != self.max_detections or self.max_detections < 1:
            raise ValueError(f"ScanDetectorParams.max_detections must be an integer >= 1, got {self.max_detections}")
        if self.subtract_map not in (False, True, 0, 1):
            raise ValueError(f"ScanDetectorParams.subtract_map must be a bool, got {self.subtract_map!r}")

    @staticmethod
    def _d2(length: float, resolution: float) -> float:
        r = np.float64(length) / np.float64(resolution)   # SensorParams.agent_d2's rounding
        with np.errstate(over="ignore"):
            return float(np.floor(r * r + 1e-9))

    def link_d2(self, resolution: float) -> int:
        """The squared link distance in cells, rounded down."""
        return int(self._d2(self.link_distance, resolution))

    def width_d2(self, resolution: float):
        """(width_d2_min, width_d2_max): the squared widths in cells, rounded down."""
        return int(self._d2(self.min_width, resolution)), int(self._d2(self.max_width, resolution))

    def range_m(self, sensor: "SensorParams") -> float:
        """The range in metres: max_range, or the sensor's marking range."""
        return float(sensor.max_range if self.max_range is None else self.max_range)

    def range_d2(self, resolution: float, sensor: "SensorParams") -> int:
        """The squared range in cells, rounded down."""
        return int(self._d2(self.range_m(sensor), resolution))

    def supported(self, resolution: float = None, sensor: "SensorParams" = None) -> bool:
        """Does the library run this detector: at most 64 rows per robot and, with a resolution, squared distances that fit
        the struct's int32 fields (the range too when `sensor` is given or max_range is set)?"""
        if self.max_detections > 64 or self.min_points >= 2 ** 31:
            return False
        if resolution is None:
            return True
        lengths = [self.link_distance, self.min_width, self.max_width]
        if sensor is not None or self.max_range is not None:
            lengths.append(self.max_range if self.max_range is not None else sensor.max_range)
        return all(np.isfinite(d) and d < 2.0 ** 31 for d in (self._d2(v, resolution) for v in lengths))


@dataclass
class PlanRepairParams:
    """Plan repair (include/smpc_plan_repair.h; BatchEpisode(repair=...)): every tick a robot whose plan runs into impassable
    cells of its own window gets the least-cost detour inside the window, spliced into its plan. radius: half the side of the
    square region around the robot that is searched, metres (at most 63 cells of the window's resolution). rejoin_clearance:
    the detour comes back to the plan at the first passable pose at least this far, metres, behind the last blocked one: a
    scan does not show an obstacle's back. stride: every stride-th cell of the detour becomes a pose. The costs are the
    global plans' (GlobalPlanParams): w = neutral_cost + cost_weight * cost, passable below lethal_min_cost, and 255 with
    allow_unknown."""
    radius: float = 3.0
    rejoin_clearance: float = 0.5
    stride: int = 2
    neutral_cost: int = 50
    cost_weight: int = 1
    lethal_min_cost: int = 253
    allow_unknown: bool = False

    MAX_RADIUS_CELLS = 63   # SMPC_REPAIR_MAX_RADIUS

    def __post_init__(self):
        if not (np.isfinite(self.radius) and self.radius > 0.0):
            raise ValueError(f"PlanRepairParams.radius must be finite and > 0, got {self.radius}")
        if not (np.isfinite(self.rejoin_clearance) and self.rejoin_clearance >= 0.0):
            raise ValueError(f"PlanRepairParams.rejoin_clearance must be finite and >= 0, got {self.rejoin_clearance}")
        if int(self.stride) != self.stride or self.stride < 1:
            raise ValueError(f"PlanRepairParams.stride must be an integer >= 1, got {self.stride}")
        if self.neutral_cost < 1 or self.cost_weight < 0 or self.neutral_cost + 255 * self.cost_weight > 65535:
            raise ValueError("PlanRepairParams: neutral_cost >= 1, cost_weight >= 0 and neutral_cost + 255 * cost_weight <= 65535")
        if not 0 <= self.lethal_min_cost <= 255:
            raise ValueError(f"PlanRepairParams.lethal_min_cost must be 0..255, got {self.lethal_min_cost}")

    def radius_cells(self, resolution: float) -> int:
        """R: the radius in cells of `resolution`, rounded down (SensorParams.agent_d2's guard against a quotient just below an
        integer), at least 1."""
        r = np.floor(np.float64(self.radius) / np.float64(resolution) + 1e-9)
        return int(max(1.0, min(r, 2.0 ** 31 - 1)))

    @property
    def clearance_d2(self) -> float:
        """The squared rejoin clearance in metres^2: one product of doubles."""
        return float(np.float64(self.rejoin_clearance) * np.float64(self.rejoin_clearance))

    def supported(self, resolution: float = None) -> bool:
        """Does the library run this repair (include/smpc_plan_repair.h's two SMPC_ERR_UNSUPPORTED)? With a resolution: a
        radius of at most 63 cells, and potentials that fit 32 bits over the region, S * S * 7 * (neutral_cost + 255 *
        cost_weight) < 2^32 - 1; without one the bound is checked for 63 cells."""
        R = self.MAX_RADIUS_CELLS if resolution is None else self.radius_cells(resolution)
        S = 2 * R + 1
        return R <= self.MAX_RADIUS_CELLS and S * S * 7 * (self.neutral_cost + 255 * self.cost_weight) < 2 ** 32 - 1


@dataclass
class PlantParams:
    """The robot plant (include/smpc_plant.h; BatchEpisode(plant=...)): every tick the selected command is executed by a
    model of the base instead of being taken for the motion. The command that was selected latency_ticks periods ago is
    clamped to the velocity bounds (OptimizerParams' v_min, v_max, w_max), the speed may grow by at most max_accel * dt and
    shrink by at most max_decel * dt in one period, the turn rate may change by max_ang_accel * dt, and the period's straight
    segment is walked in `substeps` steps that end in front of the first one that brings the disc of robot_radius closer to
    a wall cell (world cost >= wall_min_cost, 255 only with unknown_is_wall, beyond the map with outside_is_wall) or to an
    agent whose centre is within robot_radius + agent_radius. robot_radius None: no walls; agent_radius None: no agents.
    The defaults are a differential-drive base of the reference's size class: 2.5 m/s^2, 3.2 rad/s^2 (Nav2's shipped
    velocity smoother), a disc of 0.24 m (the inscribed radius of the reference's 0.48 m footprint) and persons of 0.3 m."""
    max_accel: float = 2.5
    max_decel: float = 2.5
    max_ang_accel: float = 3.2
    latency_ticks: int = 0
    substeps: int = 8
    robot_radius: float = 0.24
    agent_radius: float = 0.3
    wall_min_cost: int = 254
    unknown_is_wall: bool = False
    outside_is_wall: bool = True

    def __post_init__(self):
        for name in ("max_accel", "max_decel", "max_ang_accel"):
            v = getattr(self, name)
            if not v >= 0.0:   # +inf: no limit
                raise ValueError(f"PlantParams.{name} must be >= 0 (inf: no limit), got {v}")
        for name in ("robot_radius", "agent_radius"):
            v = getattr(self, name)
            if v is not None and not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"PlantParams.{name} must be None or finite and >= 0, got {v}")
        if int(self.latency_ticks) != self.latency_ticks or not 0 <= self.latency_ticks <= 8:
            raise ValueError(f"PlantParams.latency_ticks must be an integer in 0..8, got {self.latency_ticks}")
        if int(self.substeps) != self.substeps or not 1 <= self.substeps <= 16:
            raise ValueError(f"PlantParams.substeps must be an integer in 1..16, got {self.substeps}")
        if int(self.wall_min_cost) != self.wall_min_cost or not 0 <= self.wall_min_cost <= 255:
            raise ValueError(f"PlantParams.wall_min_cost must be 0..255, got {self.wall_min_cost}")

    @classmethod
    def ideal(cls) -> "PlantParams":
        """The plant that follows every command within the velocity bounds at once and touches nothing: infinite limits, no
        latency, no contacts, one substep."""
        inf = float("inf")
        return cls(max_accel=inf, max_decel=inf, max_ang_accel=inf, latency_ticks=0, substeps=1, robot_radius=None, agent_radius=None)

    def footprint_d2(self, resolution: float) -> int:
        """The squared footprint radius in cells, rounded down as SensorParams.agent_d2 rounds; -1 without robot_radius."""
        if self.robot_radius is None:
            return -1
        r = np.float64(self.robot_radius) / np.float64(resolution)
        return int(np.floor(r * r + 1e-9))

    def contact_dist(self) -> float:
        """robot_radius + agent_radius (a missing robot_radius counts 0); 0.0, which no distance is below, without agent_radius."""
        if self.agent_radius is None:
            return 0.0
        return float(np.float64(self.robot_radius or 0.0) + np.float64(self.agent_radius))

    def deltas(self, dt: float):
        """(dv_up, dv_down, dw) as the call takes them: acceleration * dt, one product each (inf stays inf, also with dt 0)."""
        if not (np.isfinite(dt) and dt >= 0.0):
            raise ValueError(f"PlantParams.deltas: dt must be finite and >= 0, got {dt}")
        mul = lambda a: float("inf") if np.isinf(a) else float(np.float64(a) * np.float64(dt))
        return mul(self.max_accel), mul(self.max_decel), mul(self.max_ang_accel)

    def supported(self, resolution: float = None) -> bool:
        """Does the library run this plant: with `resolution`, a footprint of at most 15 cells (footprint_d2 <= 225)?"""
        if resolution is None or self.robot_radius is None:
            return True
        r = np.float64(self.robot_radius) / np.float64(resolution)
        return bool(r * r + 1e-9 < 226.0)


MONITOR_SHAPES = {"circle": 0, "polygon": 1}
MONITOR_ACTIONS = {"stop": 0, "slowdown": 1, "limit": 2, "approach": 3}


@dataclass
class MonitorZone:
    """One zone of the collision monitor (smpc_monitor_zone of include/smpc_collision_monitor.h), in the robot's frame with x
    forward: a circle of `radius` around the robot or a polygon of 3..16 `vertices` [(x, y), ..] in either orientation, which
    triggers when at least min_points of the scan's points lie inside. action "stop": the command becomes (0, 0);
    "slowdown": it is scaled by slowdown_ratio; "limit": it is scaled so that |v| <= linear_limit and |w| <= angular_limit;
    "approach": the command is simulated over MonitorParams' horizon and scaled by the share of the horizon that passes
    before the zone, carried along, triggers."""
    action: str = "stop"
    radius: float = None
    vertices: tuple = None
    min_points: int = 4
    slowdown_ratio: float = 0.5
    linear_limit: float = 0.5
    angular_limit: float = 0.5

    def __post_init__(self):
        if self.action not in MONITOR_ACTIONS:
            raise ValueError(f"MonitorZone.action must be one of {sorted(MONITOR_ACTIONS)}, got {self.action!r}")
        if (self.radius is None) == (self.vertices is None):
            raise ValueError("MonitorZone takes a radius (a circle) or vertices (a polygon), not both and not neither")
        if self.radius is not None and not (np.isfinite(self.radius) and self.radius >= 0.0):
            raise ValueError(f"MonitorZone.radius must be finite and >= 0, got {self.radius}")
        if self.vertices is not None:
            v = np.asarray(self.vertices, np.float64)
            if v.ndim != 2 or v.shape[1] != 2 or not 3 <= v.shape[0] <= 16 or not np.isfinite(v).all():
                raise ValueError("MonitorZone.vertices must be 3..16 finite (x, y) pairs")
            self.vertices = tuple((float(x), float(y)) for x, y in v)
        if int(self.min_points) != self.min_points or self.min_points < 1:
            raise ValueError(f"MonitorZone.min_points must be an integer >= 1, got {self.min_points}")
        if not 0.0 <= self.slowdown_ratio <= 1.0:
            raise ValueError(f"MonitorZone.slowdown_ratio must lie in [0, 1], got {self.slowdown_ratio}")
        for name in ("linear_limit", "angular_limit"):
            if not getattr(self, name) >= 0.0:   # +inf: no limit
                raise ValueError(f"MonitorZone.{name} must be >= 0 (inf: no limit), got {getattr(self, name)}")

    @property
    def shape(self) -> str:
        return "circle" if self.vertices is None else "polygon"


@dataclass
class MonitorParams:
    """The collision monitor (include/smpc_collision_monitor.h; BatchEpisode(monitor=..., sensor=...)): every tick the selected
    command passes the zones, which look at the cells the tick's scan stopped at, before it reaches the base. zones: 1..8
    MonitorZone, shared by all robots. The "approach" zones simulate the command for time_before_collision seconds in steps
    of simulation_time_step: M = round(time_before_collision / simulation_time_step) steps, at most 32 (Nav2's
    collision_monitor parameters of the same names)."""
    zones: tuple = ()
    time_before_collision: float = 1.2
    simulation_time_step: float = 0.1

    def __post_init__(self):
        self.zones = tuple(self.zones)
        if not self.zones or not all(isinstance(z, MonitorZone) for z in self.zones):
            raise ValueError("MonitorParams.zones must be a non-empty sequence of MonitorZone")
        if not (np.isfinite(self.time_before_collision) and self.time_before_collision >= 0.0):
            raise ValueError(f"MonitorParams.time_before_collision must be finite and >= 0, got {self.time_before_collision}")
        if not (np.isfinite(self.simulation_time_step) and self.simulation_time_step > 0.0):
            raise ValueError(f"MonitorParams.simulation_time_step must be finite and > 0, got {self.simulation_time_step}")
        if self.steps() < 1 and any(z.action == "approach" for z in self.zones):
            raise ValueError("MonitorParams: an approach zone needs at least one simulation step (time_before_collision >= simulation_time_step / 2)")

    def steps(self) -> int:
        """M, the simulation steps of the approach zones."""
        return int(round(float(self.time_before_collision) / float(self.simulation_time_step)))

    def supported(self) -> bool:
        """Does the library run this monitor: at most 8 zones and 32 simulation steps?"""
        return len(self.zones) <= 8 and self.steps() <= 32

    @classmethod
    def nav2_like(cls, robot_radius: float = 0.24) -> "MonitorParams":
        """Three zones in the manner of Nav2's shipped collision_monitor parameters around a robot of robot_radius: a STOP
        circle a little beyond the body (1.25 radii), a SLOWDOWN polygon ahead of it (from the stop circle's rear to 5 radii
        ahead, 2 radii to either side, ratio 0.5) and an APPROACH polygon of the footprint (the octagon that circumscribes
        the disc), simulated 1.2 s ahead in steps of 0.1 s. Every zone triggers with 4 points."""
        r = float(robot_radius)
        if not (np.isfinite(r) and r > 0.0):
            raise ValueError(f"MonitorParams.nav2_like: robot_radius must be finite and > 0, got {robot_radius}")
        k = r / np.cos(np.pi / 8.0)
        footprint = tuple((float(k * np.cos(np.pi / 8.0 + i * np.pi / 4.0)), float(k * np.sin(np.pi / 8.0 + i * np.pi / 4.0))) for i in range(8))
        ahead = ((-1.25 * r, -2.0 * r), (5.0 * r, -2.0 * r), (5.0 * r, 2.0 * r), (-1.25 * r, 2.0 * r))
        return cls(zones=(MonitorZone(action="stop", radius=1.25 * r, min_points=4),
                          MonitorZone(action="slowdown", vertices=ahead, min_points=4, slowdown_ratio=0.5),
                          MonitorZone(action="approach", vertices=footprint, min_points=4)),
                   time_before_collision=1.2, simulation_time_step=0.1)


@dataclass
class SharedWorldParams:
    """One world for all robots of an episode (include/smpc_nearest.h; BatchEpisode(shared=..., pool=...)): every tick each
    robot is handed its at most max_people nearest agents within max_range (the detector's range in metres, VisibilityParams'
    default) out of one table: the shared pedestrians, followed, with robots_as_people, by the robots themselves.
    max_people None: the scenes' N."""
    max_range: float = 10.0
    max_people: int = None
    robots_as_people: bool = True

    def __post_init__(self):
        if not (np.isfinite(self.max_range) and self.max_range > 0.0):
            raise ValueError(f"SharedWorldParams.max_range must be finite and > 0, got {self.max_range}")
        if self.max_people is not None and not 1 <= int(self.max_people) <= 64:
            raise ValueError(f"SharedWorldParams.max_people must be 1..64 (SMPC_MAX_AGENTS), got {self.max_people}")

    def grid(self, world, reach: float = None):
        """The bins of the gather on `world` (scenes.World): (grid_x, grid_y, origin [2], bin_size). The origin is the
        world's; bin_size = max(max_range * (1 + 2^-20), larger side / 256), so that there are at most 256 x 256 = 65536
        bins (the library's limit); grid_x x grid_y bins cover the floor (at least one each). reach: a second range the
        same bins must serve (PoolCrowdParams.interaction_range: the pool's crowd step reads the gather's bins):
        max(max_range, reach) takes max_range's place."""
        res = float(world.resolution)
        width, height = world.cells_x * res, world.cells_y * res
        longest = self.max_range if reach is None else max(float(self.max_range), float(reach))
        bin_size = max(float(np.float64(longest) * np.float64(1.0 + 2.0 ** -20)), max(width, height) / 256.0)
        grid_x = min(256, max(1, int(np.ceil(width / bin_size))))
        grid_y = min(256, max(1, int(np.ceil(height / bin_size))))
        return grid_x, grid_y, np.asarray(world.origin, np.float64).reshape(2).copy(), bin_size


@dataclass
class OptimizerParams:
    # optimizer.* (src/optimizer.cpp:26-55, 76-83)
    linear_solver_type: str = "SPARSE_NORMAL_CHOLESKY"
    param_tol: float = 1e-15
    fn_tol: float = 1e-7
    gradient_tol: float = 1e-10
    max_iterations: int = 100
    debug_optimizer: bool = False
    control_horizon: int = 5
    parameter_block_length: int = 5
    current_path_weight: float = 1.0
    current_cmds_weight: float = 1.0
    # optimizer.weights.* (src/optimizer.cpp:57-75)
    distance_weight: float = 3.0
    social_weight: float = 1.0
    velocity_weight: float = 0.5
    angle_weight: float = 0.0
    agent_angle_weight: float = 0.5
    proxemics_weight: float = 90.0
    velocity_feasibility_weight: float = 0.5
    obstacle_weight: float = 0.0
    goal_align_weight: float = 0.0
    # trajectorizer.* read by the optimiser path (src/optimizer.cpp:84, src/path_trajectorizer.cpp:58-59)
    time_step: float = 0.05
    max_time: float = 3.0
    # literals of Optimizer::optimize (src/optimizer.cpp:238, 375-378)
    desired_linear_vel: float = 0.6
    v_min: float = 0.0
    v_max: float = 0.6
    w_min: float = -1.4
    w_max: float = 1.4
    # switches that have no reference counterpart (0 = reference behaviour)
    fixed_iterations: int = 0
    tol_needs_successful_step: int = 0

    def __post_init__(self):
        if self.linear_solver_type not in LINEAR_SOLVER:
            # same error behaviour as src/optimizer.cpp:31-45
            raise RuntimeError("Invalid parameter: linear_solver_type")

    @property
    def dt(self) -> float:
        """time_step as Optimizer::optimize sees it: a float widened to double (optimizer.hpp:170)."""
        return float(np.float32(self.time_step))

    @property
    def rollout_steps(self) -> int:
        """T for a trajectorized path longer than max_time: format_to_optimize cuts to round(max_time/dt)-1
        poses (src/optimizer.cpp:492-497) and optimize pops one velocity (:237)."""
        maxsize = int(np.round(np.float32(self.max_time) / np.float32(self.time_step)))
        return maxsize - 2

    def to_c(self) -> SmpcParams:
        p = SmpcParams()
        p.distance_w = self.distance_weight
        p.socialwork_w = self.social_weight
        p.velocity_w = self.velocity_weight
        p.angle_w = self.angle_weight
        p.agent_angle_w = self.agent_angle_weight
        p.proxemics_w = self.proxemics_weight
        p.velocity_feasibility_w = self.velocity_feasibility_weight
        p.obstacle_w = self.obstacle_weight
        p.goal_align_w = self.goal_align_weight
        p.control_horizon = int(self.control_horizon)
        p.parameter_block_length = int(self.parameter_block_length)
        p.max_iterations = int(self.max_iterations)
        p.linear_solver_type = LINEAR_SOLVER[self.linear_solver_type]
        p.fn_tol = self.fn_tol
        p.gradient_tol = self.gradient_tol
        p.param_tol = self.param_tol
        p.desired_linear_vel = self.desired_linear_vel
        p.v_min, p.v_max, p.w_min, p.w_max = self.v_min, self.v_max, self.w_min, self.w_max
        p.fixed_iterations = int(self.fixed_iterations)
        p.tol_needs_successful_step = int(self.tol_needs_successful_step)
        return p

    def scene_row(self) -> np.ndarray:
        """The 14 values one row of smpc_scene_batch.scene_params takes from this parameter set, in struct order
        (_abi.SCENE_PARAM_FIELDS): nine weights, desired_linear_vel, v_min, v_max, w_min, w_max."""
        return np.array([float(getattr(self, f)) for f in SCENE_ROW_FIELDS], dtype=np.float64)

    def dims(self, T: int, has_people: bool = True):
        """(CH, bl, nb, P, M, n_bounded) exactly as src/optimizer.cpp:248-249, 364, 373 derive them."""
        CH = min(self.control_horizon, T)
        bl = min(self.parameter_block_length, CH)
        nb = (CH - 1) // bl + 1
        nfeas = max(0, min(CH // bl, T) - 1)
        M = (8 if has_people else 5) * T + nfeas
        return CH, bl, nb, 2 * nb, M, CH // bl

    def replace(self, **kw) -> "OptimizerParams":
        d = asdict(self)
        d.update(kw)
        return OptimizerParams(**d)

    @staticmethod
    def readme() -> "OptimizerParams":
        """The parameter set of the reference's README.md:66-98 with time_step 0.05 (critics.md / benchmark yaml),
        i.e. the H=18 / bl=6 / T=28 configuration BASELINE.json's metric is quoted on."""
        return OptimizerParams(
            linear_solver_type="DENSE_SCHUR", param_tol=1e-9, fn_tol=1e-5, gradient_tol=1e-8, max_iterations=40,
            control_horizon=18, parameter_block_length=6, current_path_weight=1.0, current_cmds_weight=0.5,
            distance_weight=20.0, social_weight=120.0, velocity_weight=10.0, angle_weight=250.0,
            agent_angle_weight=40.0, velocity_feasibility_weight=5.0, goal_align_weight=10.0, obstacle_weight=0.15,
            proxemics_weight=100.0, time_step=0.05, max_time=1.5)

    @staticmethod
    def params_yaml() -> "OptimizerParams":
        """params/params.yaml:25-56 as shipped (proxemics_weight absent -> code default 90)."""
        return OptimizerParams(
            linear_solver_type="DENSE_SCHUR", param_tol=1e-9, fn_tol=1e-5, gradient_tol=1e-8, max_iterations=40,
            control_horizon=20, parameter_block_length=4, current_path_weight=1.0, current_cmds_weight=0.5,
            distance_weight=50.0, social_weight=700.0, velocity_weight=8.0, angle_weight=180.0,
            agent_angle_weight=0.0, velocity_feasibility_weight=5.0, goal_align_weight=8.0, obstacle_weight=0.2,
            time_step=0.05, max_time=2.0)

    @staticmethod
    def soc_work_obst_benchmark() -> "OptimizerParams":
        """params/soc_work_obst_parameters_in_benchmark.yaml:104-136 as shipped (proxemics_weight absent -> code default
        90; the benchmark's local costmap is 4 m x 4 m at 0.05 m = 80 x 80 cells, :143-149)."""
        return OptimizerParams(
            linear_solver_type="DENSE_SCHUR", param_tol=1e-9, fn_tol=1e-5, gradient_tol=1e-8, max_iterations=40,
            control_horizon=18, parameter_block_length=6, current_path_weight=1.0, current_cmds_weight=0.5,
            distance_weight=20.0, social_weight=120.0, velocity_weight=10.0, angle_weight=250.0,
            agent_angle_weight=40.0, velocity_feasibility_weight=5.0, goal_align_weight=10.0, obstacle_weight=0.13,
            time_step=0.05, max_time=1.5)

    @staticmethod
    def obst_only_benchmark() -> "OptimizerParams":
        """params/obst_only_parameters_in_benchmark.yaml:104-136: the same file with social_weight 0 and
        agent_angle_weight 0 (:129,132) — people are still handed to the optimiser, so the social-work and agent-angle
        rows exist with zero weight and the proxemics row keeps its code default 90."""
        return OptimizerParams.soc_work_obst_benchmark().replace(social_weight=0.0, agent_angle_weight=0.0)

    BENCHMARK_COSTMAP_CELLS = 80  # local costmap of both benchmark files: width = height = 4 m, resolution 0.05 m

    @staticmethod
    def from_yaml(path: str, plugin: str = "FollowPath") -> "OptimizerParams":
        import yaml

        with open(path, "r") as f:
            doc = yaml.load(f, Loader=yaml.SafeLoader)

        def find(node):
            if isinstance(node, dict):
                if plugin in node and isinstance(node[plugin], dict) and "optimizer" in node[plugin]:
                    return node[plugin]
                for v in node.values():
                    r = find(v)
                    if r is not None:
                        return r
            return None

        sec = find(doc)
        if sec is None:
            raise RuntimeError(f"no '{plugin}' section with an 'optimizer' block in {path}")
        opt = dict(sec.get("optimizer", {}))
        weights = dict(opt.pop("weights", {}) or {})
        traj = sec.get("trajectorizer", {}) or {}
        kw = {}
        fields = OptimizerParams.__dataclass_fields__
        for k, v in list(opt.items()) + list(weights.items()):
            if k in fields:
                kw[k] = v
        for k in ("time_step", "max_time"):
            if k in traj:
                kw[k] = traj[k]
        return OptimizerParams(**kw)


def scene_param_rows(param_sets, assignment) -> np.ndarray:
    """Rows of smpc_scene_batch.scene_params [B,14]: scene b takes param_sets[assignment[b]]'s scene_row(). The sets may
    differ only in the 14 per-scene values; anything else (control_horizon, parameter_block_length, tolerances,
    max_iterations, linear_solver_type, time_step, ...) shapes the problem or the solver loop and stays the handle's, so
    a set that differs there is refused (ValueError)."""
    param_sets = list(param_sets)
    if not param_sets:
        raise ValueError("no parameter sets")
    shared = [f.name for f in fields(OptimizerParams) if f.name not in SCENE_ROW_FIELDS]
    base = param_sets[0]
    for i, p in enumerate(param_sets[1:], 1):
        bad = [n for n in shared if getattr(p, n) != getattr(base, n)]
        if bad:
            raise ValueError(f"parameter set {i} differs from set 0 in {', '.join(bad)}: only the per-scene weights, "
                             "desired_linear_vel and velocity bounds may differ within one batch")
    assignment = np.asarray(assignment)
    if assignment.ndim != 1 or not np.issubdtype(assignment.dtype, np.integer):
        raise ValueError("assignment must be a 1-D integer array")
    if assignment.size and (assignment.min() < 0 or assignment.max() >= len(param_sets)):
        raise ValueError("assignment indexes outside the parameter sets")
    table = np.stack([p.scene_row() for p in param_sets])
    return np.ascontiguousarray(table[assignment])


def check_scene_param_rows(rows, B: int) -> np.ndarray:
    """rows as the [B,14] float64 array smpc_scene_batch.scene_params takes, checked as the library checks host rows:
    every value finite, v_min <= v_max and w_min <= w_max (ValueError otherwise). For callers that hand the rows over as
    device memory, which the library does not check."""
    sp = np.ascontiguousarray(rows, np.float64)
    if sp.shape != (B, len(SCENE_PARAM_FIELDS)):
        raise ValueError(f"scene_params: expected shape {(B, len(SCENE_PARAM_FIELDS))}, got {sp.shape}")
    col = {f: i for i, f in enumerate(SCENE_PARAM_FIELDS)}
    if not np.isfinite(sp).all():
        raise ValueError("scene_params: every value must be finite")
    if not ((sp[:, col["v_min"]] <= sp[:, col["v_max"]]).all() and (sp[:, col["w_min"]] <= sp[:, col["w_max"]]).all()):
        raise ValueError("scene_params: needs v_min <= v_max and w_min <= w_max")
    return sp
