"""Scene batches for the batched MPC solver: the inputs `Optimizer::optimize` hands to the Ceres problem
(reference src/optimizer.cpp:197-237) in structure-of-arrays form, plus the seeded synthetic crowd-scene
generator SURVEY.md §8(d) specifies (counter-based SplitMix64 keyed by (seed, scene_id, field_id), so every
shard / the CPU oracle regenerate identical scenes with no communication).
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._abi import SCENE_PARAM_FIELDS, SmpcSceneBatch
from .params import OptimizerParams

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)
SCENE_PARAM_COUNT = len(SCENE_PARAM_FIELDS)  # doubles per row of SceneBatch.scene_params


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = (x + np.uint64(0x9E3779B97F4A7C15)) & _MASK
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK
        return z ^ (z >> np.uint64(31))


def uniform(seed: int, scene_ids: np.ndarray, field_id: int, n: int = 1) -> np.ndarray:
    """U[0,1) doubles of shape [len(scene_ids), n], a pure function of (seed, scene_id, field_id, k)."""
    sid = scene_ids.astype(np.uint64)[:, None]
    k = np.arange(n, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        key = _splitmix64(np.uint64(seed) ^ _splitmix64(sid * np.uint64(0x100000001B3) + np.uint64(field_id)))
        bits = _splitmix64(key + k * np.uint64(0xD1342543DE82EF95))
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


@dataclass
class SceneBatch:
    """SoA inputs of B independent MPC problems (layout = include/smpc.h `smpc_scene_batch`)."""
    T: int
    N: int
    dt: float
    pose0: np.ndarray          # [B,3]
    init_params: np.ndarray    # [B,P]
    path_pts: np.ndarray       # [B,T+1,2]
    goal_yaw: np.ndarray       # [B]
    people: np.ndarray         # [B,T+1,6,N]
    has_people: np.ndarray     # [B] uint8
    costmap: np.ndarray        # [B or 1,size_y,size_x] uint8
    costmap_origin: np.ndarray  # [B or 1,2]
    resolution: float
    costmap_shared: bool = False
    # optional horizon of each scene, 1 <= T_scene[b] <= T (smpc_scene_batch.T_scene): of path_pts / people the first
    # T_scene[b] + 1 rows of scene b count, of init_params the first P_b entries; None: every scene has T steps
    T_scene: Optional[np.ndarray] = None
    # optional critic weights, target speed and velocity bounds of each scene [B,14] float64 in smpc_scene_params order
    # (smpc_scene_batch.scene_params; params.scene_param_rows builds them); None: every scene takes the handle's values
    scene_params: Optional[np.ndarray] = None

    @property
    def B(self) -> int:
        return int(self.pose0.shape[0])

    @property
    def size_y(self) -> int:
        return int(self.costmap.shape[1])

    @property
    def size_x(self) -> int:
        return int(self.costmap.shape[2])

    def validate(self, P: int):
        B, T, N = self.B, self.T, self.N
        assert self.pose0.shape == (B, 3) and self.pose0.dtype == np.float64
        assert self.init_params.shape == (B, P) and self.init_params.dtype == np.float64
        assert self.path_pts.shape == (B, T + 1, 2) and self.path_pts.dtype == np.float64
        assert self.goal_yaw.shape == (B,) and self.goal_yaw.dtype == np.float64
        assert self.people.shape == (B, T + 1, 6, N) and self.people.dtype == np.float64
        assert self.has_people.shape == (B,) and self.has_people.dtype == np.uint8
        nb_maps = 1 if self.costmap_shared else B
        assert self.costmap.shape[0] == nb_maps and self.costmap.dtype == np.uint8
        assert self.costmap_origin.shape == (nb_maps, 2) and self.costmap_origin.dtype == np.float64
        for a in (self.pose0, self.init_params, self.path_pts, self.goal_yaw, self.people, self.has_people,
                  self.costmap, self.costmap_origin):
            assert a.flags["C_CONTIGUOUS"]
        if self.T_scene is not None:
            assert self.T_scene.shape == (B,) and self.T_scene.dtype == np.int32 and self.T_scene.flags["C_CONTIGUOUS"]
        if self.scene_params is not None:
            assert (self.scene_params.shape == (B, SCENE_PARAM_COUNT) and self.scene_params.dtype == np.float64
                    and self.scene_params.flags["C_CONTIGUOUS"])

    def to_c(self) -> SmpcSceneBatch:
        """C view over the host arrays (arrays stay owned by this object)."""
        sb = SmpcSceneBatch()
        sb.B, sb.T, sb.N, sb.on_device = self.B, self.T, self.N, 0
        sb.dt = self.dt
        sb.pose0 = self.pose0.ctypes.data
        sb.init_params = self.init_params.ctypes.data
        sb.path_pts = self.path_pts.ctypes.data
        sb.goal_yaw = self.goal_yaw.ctypes.data
        sb.people = self.people.ctypes.data
        sb.has_people = self.has_people.ctypes.data
        sb.costmap = self.costmap.ctypes.data
        sb.costmap_shared = 1 if self.costmap_shared else 0
        sb.size_x, sb.size_y = self.size_x, self.size_y
        sb.costmap_origin = self.costmap_origin.ctypes.data
        sb.resolution = self.resolution
        if self.T_scene is not None:
            sb.T_scene = self.T_scene.ctypes.data
        if self.scene_params is not None:
            sb.scene_params = self.scene_params.ctypes.data
        return sb

    def to_device(self, device="cuda:0"):
        """Copy to HBM as torch tensors; returns (SmpcSceneBatch with device pointers, dict of tensors)."""
        import torch

        t = {k: torch.from_numpy(getattr(self, k)).to(device) for k in
             ("pose0", "init_params", "path_pts", "goal_yaw", "people", "has_people", "costmap", "costmap_origin")}
        if self.T_scene is not None:
            t["T_scene"] = torch.from_numpy(self.T_scene).to(device)
        if self.scene_params is not None:
            t["scene_params"] = torch.from_numpy(self.scene_params).to(device)
        sb = SmpcSceneBatch()
        sb.B, sb.T, sb.N, sb.on_device = self.B, self.T, self.N, 1
        sb.dt = self.dt
        for k, v in t.items():
            setattr(sb, k, v.data_ptr())
        sb.costmap_shared = 1 if self.costmap_shared else 0
        sb.size_x, sb.size_y = self.size_x, self.size_y
        sb.resolution = self.resolution
        return sb, t

    def select(self, idx) -> "SceneBatch":
        idx = np.atleast_1d(np.asarray(idx))
        cm = self.costmap if self.costmap_shared else np.ascontiguousarray(self.costmap[idx])
        co = self.costmap_origin if self.costmap_shared else np.ascontiguousarray(self.costmap_origin[idx])
        return SceneBatch(self.T, self.N, self.dt, np.ascontiguousarray(self.pose0[idx]),
                          np.ascontiguousarray(self.init_params[idx]), np.ascontiguousarray(self.path_pts[idx]),
                          np.ascontiguousarray(self.goal_yaw[idx]), np.ascontiguousarray(self.people[idx]),
                          np.ascontiguousarray(self.has_people[idx]), cm, co, self.resolution, self.costmap_shared,
                          None if self.T_scene is None else np.ascontiguousarray(self.T_scene[idx]),
                          None if self.scene_params is None else np.ascontiguousarray(self.scene_params[idx]))

    def with_horizons(self, T_scene) -> "SceneBatch":
        """The same scenes with a horizon per scene: scene b keeps its first T_scene[b] + 1 poses / people rows; its goal
        heading becomes the heading the path has at its own last pose (scenes built by make_scenes: the reference path
        is an arc, so that is the heading after T_scene[b] steps)."""
        T_scene = np.ascontiguousarray(T_scene, np.int32)
        assert T_scene.shape == (self.B,) and T_scene.min() >= 1 and T_scene.max() <= self.T
        out = self.select(np.arange(self.B))
        out.T_scene = T_scene
        return out

    def cut(self, idx, Tb: int, P_b: int) -> "SceneBatch":
        """Scenes idx as a batch whose T is Tb: what a caller with exactly these horizons would hand over (arrays
        truncated to Tb + 1 rows and P_b parameters)."""
        sub = self.select(idx)
        return SceneBatch(Tb, self.N, self.dt, sub.pose0, np.ascontiguousarray(sub.init_params[:, :P_b]),
                          np.ascontiguousarray(sub.path_pts[:, :Tb + 1]), sub.goal_yaw,
                          np.ascontiguousarray(sub.people[:, :Tb + 1]), sub.has_people, sub.costmap, sub.costmap_origin,
                          self.resolution, self.costmap_shared, scene_params=sub.scene_params)

    def with_scene_params(self, scene_params) -> "SceneBatch":
        """The same scenes with weights and velocity bounds per scene (rows [B,14], e.g. from params.scene_param_rows);
        None: the handle's for every scene."""
        out = self.select(np.arange(self.B))
        out.scene_params = None if scene_params is None else np.ascontiguousarray(scene_params, np.float64)
        out.validate(self.init_params.shape[1])
        return out

    def save(self, path: str):
        extra = {} if self.scene_params is None else {"scene_params": self.scene_params}
        np.savez_compressed(path, T=self.T, N=self.N, dt=self.dt, pose0=self.pose0, init_params=self.init_params,
                            path_pts=self.path_pts, goal_yaw=self.goal_yaw, people=self.people,
                            has_people=self.has_people, costmap=self.costmap, costmap_origin=self.costmap_origin,
                            resolution=self.resolution, costmap_shared=self.costmap_shared, **extra)

    @staticmethod
    def load(path: str) -> "SceneBatch":
        z = np.load(path, allow_pickle=False)
        return SceneBatch(int(z["T"]), int(z["N"]), float(z["dt"]), z["pose0"], z["init_params"], z["path_pts"],
                          z["goal_yaw"], z["people"], z["has_people"], z["costmap"], z["costmap_origin"],
                          float(z["resolution"]), bool(z["costmap_shared"]),
                          scene_params=np.ascontiguousarray(z["scene_params"]) if "scene_params" in z.files else None)


def make_scenes(params: OptimizerParams, B: int, N: int, seed: int = 0x5EED0001, first_scene: int = 0,
                T: Optional[int] = None, map_cells: int = 200, resolution: float = 0.05,
                standing_fraction: float = 0.2, people_present: bool = True,
                n_valid: Optional[int] = None) -> SceneBatch:
    """Synthetic crowd scenes per SURVEY.md §8(d).

    pose0 near the costmap centre, a constant-curvature reference path (mirrors the trajectorizer output),
    initial parameter blocks reproducing the aliasing quirk (src/optimizer.cpp:254-261: blocks start from the
    speeds at *time steps* 0,1,2,...), constant-velocity people, u8 costmap with inflated discs.
    `n_valid` (<= N) marks agents n_valid..N-1 invalid (t = -1 at the origin), like people_to_status pads.
    """
    if T is None:
        T = params.rollout_steps
    dt = params.dt
    CH, bl, nb, P, M, _ = params.dims(T, True)
    ids = np.arange(first_scene, first_scene + B, dtype=np.int64)
    u = lambda fid, n=1: uniform(seed, ids, fid, n)

    side = map_cells * resolution
    origin = (u(1, 2) - 0.5) * 10.0                      # costmap origin, a few metres from the world origin
    centre = origin + 0.5 * side
    pos0 = centre + (u(2, 2) - 0.5)                       # centre + U(-0.5,0.5)^2
    yaw0 = (u(3)[:, 0] * 2.0 - 1.0) * np.pi
    v_cur = u(4)[:, 0] * 0.6
    w_cur = u(5)[:, 0] - 0.5
    w_ref = (u(6)[:, 0] * 2.0 - 1.0) * 0.6
    pose0 = np.stack([pos0[:, 0], pos0[:, 1], yaw0], axis=1)

    # reference path: unicycle rollout with v = 0.6, w = w_ref, T+1 poses starting at pose0
    path = np.zeros((B, T + 1, 2))
    x, y, th = pos0[:, 0].copy(), pos0[:, 1].copy(), yaw0.copy()
    path[:, 0, 0], path[:, 0, 1] = x, y
    for k in range(1, T + 1):
        x = x + 0.6 * np.cos(th) * dt
        y = y + 0.6 * np.sin(th) * dt
        th = th + w_ref * dt
        path[:, k, 0], path[:, k, 1] = x, y
    goal_yaw = th - w_ref * dt  # yaw of the last pose (pose T has heading after T-1 turns)

    init = np.zeros((B, P))
    init[:, 0], init[:, 1] = v_cur, w_cur
    for b in range(1, nb):
        init[:, 2 * b], init[:, 2 * b + 1] = 0.6, w_ref

    people = np.zeros((B, T + 1, 6, max(N, 1)))
    if N > 0:
        r = 0.8 + u(10, N) * 2.7
        phi = (u(11, N) * 2.0 - 1.0) * np.pi
        heading = (u(12, N) * 2.0 - 1.0) * np.pi
        standing = u(13, N) < standing_fraction
        lv = np.where(standing, 0.0, 0.2 + u(14, N))
        px0 = pos0[:, 0:1] + r * np.cos(phi)
        py0 = pos0[:, 1:2] + r * np.sin(phi)
        for k in range(T + 1):
            people[:, k, 0, :] = px0 + lv * np.cos(heading) * (k * dt)
            people[:, k, 1, :] = py0 + lv * np.sin(heading) * (k * dt)
            people[:, k, 2, :] = heading
            people[:, k, 3, :] = k * dt
            people[:, k, 4, :] = lv
            people[:, k, 5, :] = 0.0
        if n_valid is not None and n_valid < N:
            people[:, :, :, n_valid:] = 0.0
            people[:, :, 3, n_valid:] = -1.0
    people = np.ascontiguousarray(people[:, :, :, :N]) if N > 0 else np.zeros((B, T + 1, 6, 0))
    has_people = np.full(B, 1 if (people_present and N > 0) else 0, dtype=np.uint8)

    # costmap: K ~ U{3..8} discs (cost 254) with exponential inflation 252*exp(-3 d) out to 0.7 m
    costmap = np.zeros((B, map_cells, map_cells), dtype=np.uint8)
    K = 3 + np.floor(u(20)[:, 0] * 6.0).astype(np.int64)
    win = int(np.ceil((0.5 + 0.7) / resolution)) + 1
    offs = np.arange(-win, win + 1)
    for k in range(8):
        cr = 0.15 + u(21 + 4 * k)[:, 0] * 0.35
        # disc centre: anywhere in the map but >= 1.0 m from the start position
        ang = u(22 + 4 * k)[:, 0] * 2.0 * np.pi
        dist = 1.0 + u(23 + 4 * k)[:, 0] * (0.5 * side - 1.2)
        cx = pos0[:, 0] + dist * np.cos(ang)
        cy = pos0[:, 1] + dist * np.sin(ang)
        active = k < K
        ci = np.floor((cx - origin[:, 0]) / resolution).astype(np.int64)
        cj = np.floor((cy - origin[:, 1]) / resolution).astype(np.int64)
        ii = ci[:, None] + offs[None, :]             # x cells [B,W]
        jj = cj[:, None] + offs[None, :]             # y cells [B,W]
        wx = origin[:, 0:1] + (ii + 0.5) * resolution
        wy = origin[:, 1:2] + (jj + 0.5) * resolution
        d = np.sqrt((wx[:, None, :] - cx[:, None, None]) ** 2 + (wy[:, :, None] - cy[:, None, None]) ** 2) - cr[:, None, None]
        cost = np.where(d <= 0.0, 254.0, np.where(d <= 0.7, np.floor(252.0 * np.exp(-3.0 * d)), 0.0))
        cost = np.where(active[:, None, None], cost, 0.0).astype(np.uint8)
        inb = (ii[:, None, :] >= 0) & (ii[:, None, :] < map_cells) & (jj[:, :, None] >= 0) & (jj[:, :, None] < map_cells)
        bi = np.broadcast_to(np.arange(B)[:, None, None], cost.shape)[inb]
        yi = np.broadcast_to(jj[:, :, None], cost.shape)[inb]
        xi = np.broadcast_to(ii[:, None, :], cost.shape)[inb]
        # (b, y, x) triples are unique within one disc, so a gather / max / scatter is exact
        costmap[bi, yi, xi] = np.maximum(costmap[bi, yi, xi], cost[inb])

    sb = SceneBatch(T, N, dt, np.ascontiguousarray(pose0), np.ascontiguousarray(init), np.ascontiguousarray(path),
                    np.ascontiguousarray(goal_yaw), people, has_people, costmap, np.ascontiguousarray(origin),
                    resolution, False)
    sb.validate(P)
    return sb


def crowd_waypoints(scenes: SceneBatch, K: int = 2, seed: int = 0x5EED0002, first_scene: int = 0, margin: float = 0.5,
                    tries: int = 16):
    """Waypoint lists for the persons of `scenes` (BatchEpisode(crowd=..., person_waypoints=..., person_n_waypoints=...)):
    (waypoints [B,N,K,2], n_waypoints [B,N]), a pure function of (seed, scene id, person, slot) through `uniform`.
    Every waypoint lies inside the scene's costmap, at least `margin` from its border, on a free cell (cost 0). The first
    one lies straight ahead of the person's initial velocity, 0.5 .. 6 m away, so an episode starts the way the
    constant-velocity crowd does; the others are anywhere on the map. Each is the first of `tries` seeded candidates that
    qualifies (the first one falls back to the candidates of the others, all of them to the free cell nearest the map's
    centre). A person that stands at the start, or an invalid row, gets no waypoints: it stays where it is and only
    gives way."""
    B, N = scenes.B, scenes.N
    ids = np.arange(first_scene, first_scene + B, dtype=np.int64)
    res, sx, sy = scenes.resolution, scenes.size_x, scenes.size_y
    cm = np.broadcast_to(scenes.costmap, (B, sy, sx)) if scenes.costmap_shared else scenes.costmap
    origin = np.broadcast_to(scenes.costmap_origin, (B, 2)) if scenes.costmap_shared else scenes.costmap_origin
    st0 = scenes.people[:, 0]                                             # [B,6,N]
    rows = np.arange(B)[:, None, None]

    def qualifies(x, y):                                                  # [B,N,tries] world points
        inside = ((x >= origin[:, 0, None, None] + margin) & (x <= origin[:, 0, None, None] + sx * res - margin) &
                  (y >= origin[:, 1, None, None] + margin) & (y <= origin[:, 1, None, None] + sy * res - margin))
        cx = np.clip(np.floor((x - origin[:, 0, None, None]) / res).astype(np.int64), 0, sx - 1)
        cy = np.clip(np.floor((y - origin[:, 1, None, None]) / res).astype(np.int64), 0, sy - 1)
        return inside & (cm[rows, cy, cx] == 0)

    def first_of(x, y, ok, fx, fy):                                       # the first qualifying candidate, else (fx, fy)
        pick = np.argmax(ok, axis=2)[:, :, None]
        any_ok = ok.any(axis=2)
        return (np.where(any_ok, np.take_along_axis(x, pick, 2)[:, :, 0], fx),
                np.where(any_ok, np.take_along_axis(y, pick, 2)[:, :, 0], fy))

    # last resort: the free cell nearest the map's centre (its centre point)
    jj, ii = np.meshgrid(np.arange(sy), np.arange(sx), indexing="ij")
    d2 = (ii + 0.5 - 0.5 * sx) ** 2 + (jj + 0.5 - 0.5 * sy) ** 2
    flat = np.argmin(np.where(cm == 0, d2[None], np.inf).reshape(B, -1), axis=1)
    last_x = (origin[:, 0] + ((flat % sx) + 0.5) * res)[:, None]
    last_y = (origin[:, 1] + ((flat // sx) + 0.5) * res)[:, None]

    wp = np.zeros((B, N, K, 2))
    anywhere = []
    for k in range(K):
        ux = uniform(seed, ids, 200 + 2 * k, N * tries).reshape(B, N, tries)
        uy = uniform(seed, ids, 201 + 2 * k, N * tries).reshape(B, N, tries)
        x = origin[:, 0, None, None] + margin + ux * (sx * res - 2.0 * margin)
        y = origin[:, 1, None, None] + margin + uy * (sy * res - 2.0 * margin)
        anywhere.append(first_of(x, y, qualifies(x, y), last_x, last_y))
    dist = 0.5 + 5.5 * uniform(seed, ids, 199, N * tries).reshape(B, N, tries)
    x = st0[:, 0, :, None] + dist * np.cos(st0[:, 2, :, None])
    y = st0[:, 1, :, None] + dist * np.sin(st0[:, 2, :, None])
    wp[:, :, 0, 0], wp[:, :, 0, 1] = first_of(x, y, qualifies(x, y), *anywhere[0])
    for k in range(1, K):
        wp[:, :, k, 0], wp[:, :, k, 1] = anywhere[k]
    walking = (st0[:, 3, :] != -1.0) & (st0[:, 4, :] > 0.0)
    n_wp = np.where(walking, K, 0).astype(np.int32)
    return np.ascontiguousarray(wp), np.ascontiguousarray(n_wp)


def crowd_groups(scenes: SceneBatch, sizes=(2, 3), share: float = 0.5, K: int = 2, seed: int = 0x5EED0003,
                 first_scene: int = 0, **waypoint_options):
    """Pedestrian groups for the persons of `scenes` (BatchEpisode(crowd=..., person_groups=...)): (group_id [B,N] int32,
    waypoints [B,N,K,2], n_waypoints [B,N]), a pure function of (seed, scene id) through `uniform`, so the result for a
    slice of the scenes (first_scene) is the slice of the result. Of a scene's walking persons, taken in row order, the
    first floor(share * their number) go into groups of consecutive rows whose sizes are drawn from `sizes` (a size
    that no longer fits is replaced by the largest one that does; what is left below the smallest size stays alone).
    A scene's groups are numbered 0, 1, ...; a standing person, an invalid row and everybody else get -1. The waypoints
    are crowd_waypoints' (waypoint_options are passed on), except that a group's members share their first member's
    list: companions head for the same places."""
    B, N = scenes.B, scenes.N
    sizes = sorted(int(s) for s in sizes)
    if not sizes or sizes[0] < 2 or not 0.0 <= share <= 1.0:
        raise ValueError("crowd_groups: sizes >= 2 and 0 <= share <= 1")
    wp, n_wp = crowd_waypoints(scenes, K=K, first_scene=first_scene, **waypoint_options)
    ids = np.arange(first_scene, first_scene + B, dtype=np.int64)
    draw = uniform(seed, ids, 300, max(N, 1))
    st0 = scenes.people[:, 0]
    walking = (st0[:, 3, :] != -1.0) & (st0[:, 4, :] > 0.0)
    gid = np.full((B, N), -1, np.int32)
    for b in range(B):
        rows = np.flatnonzero(walking[b])
        quota, at, g = int(np.floor(share * len(rows))), 0, 0
        while True:
            fits = [s for s in sizes if s <= quota]
            if not fits:
                break
            size = sizes[int(draw[b, g] * len(sizes))]
            size = size if size <= quota else fits[-1]
            members = rows[at:at + size]
            gid[b, members] = g
            wp[b, members] = wp[b, members[0]]
            n_wp[b, members] = n_wp[b, members[0]]
            quota, at, g = quota - size, at + size, g + 1
    return gid, np.ascontiguousarray(wp), np.ascontiguousarray(n_wp)


# -- a world map and the rolling local costmaps cut out of it (include/smpc_local_costmap.h) ------------------------------
@dataclass
class World:
    """The map a closed-loop episode's rolling local costmaps are cut out of (BatchEpisode(world=...))."""
    map: np.ndarray        # [Hy,Hx] uint8 costs
    origin: np.ndarray     # [2] world coordinates of the corner of cell (0,0)
    resolution: float

    @property
    def cells_y(self) -> int:
        return int(self.map.shape[0])

    @property
    def cells_x(self) -> int:
        return int(self.map.shape[1])


_CELL_LIMIT = 2.0 ** 30


def window_cells(origin, resolution: float, cell, pose_xy, size_x: int, size_y: int, force: bool = False):
    """The cell rule of smpc_local_costmap_batch on host arrays: origin [2] or [B,2] (the world's), cell [B,2] int32 (the
    world cell of every window's cell (0,0); taken as zeros under `force`), pose_xy [B,2]. Returns (cell' [B,2] int32,
    costmap_origin [B,2], moved [B] int32: 0 kept, 1 moved or forced, 2 pose not finite). numpy rounds every operation
    on its own, which is the contract."""
    res = np.float64(resolution)
    w0 = np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 2), np.shape(pose_xy))
    pose_xy = np.asarray(pose_xy, np.float64)
    cell = np.zeros(pose_xy.shape, np.int32) if force else np.asarray(cell, np.int32)
    size = np.array([size_x, size_y], np.float64)
    finite = np.isfinite(pose_xy).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        o = w0 + cell.astype(np.float64) * res
        want = pose_xy - ((size - 1.0 + 0.5) * res) / 2.0
        d = np.trunc((want - o) / res)
        c = cell.astype(np.float64) + d
        c = np.where(c > _CELL_LIMIT, _CELL_LIMIT, c)
        c = np.where(c >= -_CELL_LIMIT, c, -_CELL_LIMIT)
    new = np.where(finite[:, None], c, cell).astype(np.int32)
    changed = (new != cell).any(axis=1)
    moved = np.where(finite, (changed | force).astype(np.int32), 2).astype(np.int32)
    return new, w0 + new.astype(np.float64) * res, moved


def crop_windows(world_map: np.ndarray, cell: np.ndarray, size_x: int, size_y: int, outside_cost: int = 255) -> np.ndarray:
    """costmap [B,size_y,size_x]: window cell (y, x) of robot b is world_map[cell[b,1] + y, cell[b,0] + x] where that cell
    exists, else outside_cost. world_map [Hy,Hx] (one for all) or [B,Hy,Hx]."""
    world_map = np.asarray(world_map, np.uint8)
    cell = np.asarray(cell, np.int64)
    B = cell.shape[0]
    Hy, Hx = world_map.shape[-2:]
    wy = cell[:, 1, None] + np.arange(size_y)[None, :]   # [B,size_y]
    wx = cell[:, 0, None] + np.arange(size_x)[None, :]   # [B,size_x]
    inside = ((wy >= 0) & (wy < Hy))[:, :, None] & ((wx >= 0) & (wx < Hx))[:, None, :]
    yy, xx = np.clip(wy, 0, Hy - 1)[:, :, None], np.clip(wx, 0, Hx - 1)[:, None, :]
    got = world_map[yy, xx] if world_map.ndim == 2 else world_map[np.arange(B)[:, None, None], yy, xx]
    return np.ascontiguousarray(np.where(inside, got, np.uint8(outside_cost)).astype(np.uint8))


def make_world(cells_x: int, cells_y: int, resolution: float = 0.05, seed: int = 0x5EED0004, origin=(0.0, 0.0),
               discs: Optional[int] = None, wall_cells: int = 2) -> World:
    """A seeded floor of cells_x x cells_y cells: the discs of make_scenes' costmaps (cost 254, radius 0.15 .. 0.5 m, with
    the exponential inflation 252 exp(-3 d) out to 0.7 m), `discs` of them anywhere on the floor (default: make_scenes'
    mean density, 5.5 per 100 m^2), inside a lethal border wall of wall_cells cells, inflated the same way. A pure
    function of its arguments through `uniform`."""
    origin = np.asarray(origin, np.float64).reshape(2)
    width, height = cells_x * resolution, cells_y * resolution
    if discs is None:
        discs = int(round(5.5 * width * height / 100.0))
    ids = np.zeros(1, np.int64)
    inflate = lambda d: np.where(d <= 0.0, 254.0, np.where(d <= 0.7, np.floor(252.0 * np.exp(-3.0 * d)), 0.0))
    wx = origin[0] + (np.arange(cells_x) + 0.5) * resolution
    wy = origin[1] + (np.arange(cells_y) + 0.5) * resolution
    # the wall: cells within wall_cells of the border; d from a cell's centre to the wall's inner face
    k = np.minimum(np.minimum(np.arange(cells_x), cells_x - 1 - np.arange(cells_x))[None, :],
                   np.minimum(np.arange(cells_y), cells_y - 1 - np.arange(cells_y))[:, None]) - wall_cells
    cost = np.where(k < 0, 254.0, inflate((k + 0.5) * resolution))
    if discs > 0:
        cr = 0.15 + uniform(seed, ids, 1, discs)[0] * 0.35
        cx = origin[0] + uniform(seed, ids, 2, discs)[0] * width
        cy = origin[1] + uniform(seed, ids, 3, discs)[0] * height
        for r, x, y in zip(cr, cx, cy):
            d = np.sqrt((wx[None, :] - x) ** 2 + (wy[:, None] - y) ** 2) - r
            cost = np.maximum(cost, inflate(d))
    return World(np.ascontiguousarray(cost.astype(np.uint8)), origin, float(resolution))


def scenes_in_world(params: OptimizerParams, world: World, B: int, N: int, seed: int = 0x5EED0001, size_x: int = 200,
                    size_y: int = 200, first_scene: int = 0, margin: float = 1.0, people_reach: float = 3.5, tries: int = 32,
                    outside_cost: int = 255, **scene_options) -> SceneBatch:
    """B robots on `world`, each with a rolling local costmap of size_x x size_y cells: make_scenes' robots, reference
    paths and people (scene_options are passed on), moved as a whole to a seeded start position each: the first of `tries`
    candidates, uniform over the floor at least `margin` from its border, that lies on a free cell (cost 0: beyond the
    inflation of every disc and of the wall); without one, the centre of the free cell nearest the floor's centre.
    people_reach: the largest start distance of a person from its robot: make_scenes' 0.8 .. 3.5 m are mapped linearly
    onto 0.8 .. people_reach along each person's own bearing (a crowd that fits a small floor; the velocities stay). costmap / costmap_origin are the initial windows by
    smpc_local_costmap_batch's contract (window_cells from cell (0,0), crop_windows), costmap_shared = 0: a one-shot solve
    on the batch sees what the first tick of BatchEpisode(world=world) sees."""
    sc = make_scenes(params, B, N, seed=seed, first_scene=first_scene, map_cells=2, resolution=world.resolution, **scene_options)
    ids = np.arange(first_scene, first_scene + B, dtype=np.int64)
    res, Hx, Hy = world.resolution, world.cells_x, world.cells_y
    x = world.origin[0] + margin + uniform(seed, ids, 400, tries) * (Hx * res - 2.0 * margin)    # [B,tries]
    y = world.origin[1] + margin + uniform(seed, ids, 401, tries) * (Hy * res - 2.0 * margin)
    ci = np.clip(np.floor((x - world.origin[0]) / res).astype(np.int64), 0, Hx - 1)
    cj = np.clip(np.floor((y - world.origin[1]) / res).astype(np.int64), 0, Hy - 1)
    ok = world.map[cj, ci] == 0
    jj, ii = np.meshgrid(np.arange(Hy), np.arange(Hx), indexing="ij")
    flat = int(np.argmin(np.where(world.map == 0, (ii + 0.5 - 0.5 * Hx) ** 2 + (jj + 0.5 - 0.5 * Hy) ** 2, np.inf)))
    pick = np.argmax(ok, axis=1)[:, None]
    sx = np.where(ok.any(axis=1), np.take_along_axis(x, pick, 1)[:, 0], world.origin[0] + ((flat % Hx) + 0.5) * res)
    sy = np.where(ok.any(axis=1), np.take_along_axis(y, pick, 1)[:, 0], world.origin[1] + ((flat // Hx) + 0.5) * res)
    start = np.stack([sx, sy], axis=1)
    old = sc.pose0[:, 0:2].copy()
    sc.pose0[:, 0:2] = start
    sc.path_pts += (start - old)[:, None, :]
    if N > 0:
        valid = sc.people[:, :, 3:4, :] != -1.0                                     # [B,T+1,1,N]
        first = sc.people[:, 0:1, 0:2, :] - old[:, None, :, None]                   # offsets at step 0
        r = np.hypot(first[:, :, 0:1, :], first[:, :, 1:2, :])
        scale = np.where(r > 0.0, (0.8 + (r - 0.8) * ((float(people_reach) - 0.8) / 2.7)) / np.where(r > 0.0, r, 1.0), 1.0)
        moved = start[:, None, :, None] + scale * first + (sc.people[:, :, 0:2, :] - sc.people[:, 0:1, 0:2, :])
        sc.people[:, :, 0:2, :] = np.where(valid, moved, sc.people[:, :, 0:2, :])
    cell, origin, _ = window_cells(world.origin, res, None, start, size_x, size_y, force=True)
    sc.costmap = crop_windows(world.map, cell, size_x, size_y, outside_cost)
    sc.costmap_origin = np.ascontiguousarray(origin)
    sc.costmap_shared = False
    sc.validate(sc.init_params.shape[1])
    return sc


def world_goals(world: World, start_xy: np.ndarray, seed: int = 0x5EED0005, margin: float = 1.0, min_dist: float = 3.0,
                tries: int = 32) -> np.ndarray:
    """goal [B,2]: where each robot of start_xy [B,2] is sent on `world` (BatchEpisode(planner=..., goal=...)): the first of
    `tries` candidates, uniform over the floor at least `margin` from its border, that lies on a free cell (cost 0) at least
    min_dist from the robot's start; without one, the centre of the free cell nearest the floor's centre. A pure function
    of its arguments through `uniform` (fields 1 and 2, keyed by the robot's index)."""
    start_xy = np.asarray(start_xy, np.float64).reshape(-1, 2)
    ids = np.arange(start_xy.shape[0], dtype=np.int64)
    res, Hx, Hy = world.resolution, world.cells_x, world.cells_y
    x = world.origin[0] + margin + uniform(seed, ids, 1, tries) * (Hx * res - 2.0 * margin)    # [B,tries]
    y = world.origin[1] + margin + uniform(seed, ids, 2, tries) * (Hy * res - 2.0 * margin)
    ci = np.clip(np.floor((x - world.origin[0]) / res).astype(np.int64), 0, Hx - 1)
    cj = np.clip(np.floor((y - world.origin[1]) / res).astype(np.int64), 0, Hy - 1)
    ok = (world.map[cj, ci] == 0) & (np.hypot(x - start_xy[:, 0:1], y - start_xy[:, 1:2]) >= min_dist)
    jj, ii = np.meshgrid(np.arange(Hy), np.arange(Hx), indexing="ij")
    flat = int(np.argmin(np.where(world.map == 0, (ii + 0.5 - 0.5 * Hx) ** 2 + (jj + 0.5 - 0.5 * Hy) ** 2, np.inf)))
    pick = np.argmax(ok, axis=1)[:, None]
    gx = np.where(ok.any(axis=1), np.take_along_axis(x, pick, 1)[:, 0], world.origin[0] + ((flat % Hx) + 0.5) * res)
    gy = np.where(ok.any(axis=1), np.take_along_axis(y, pick, 1)[:, 0], world.origin[1] + ((flat // Hx) + 0.5) * res)
    return np.ascontiguousarray(np.stack([gx, gy], axis=1))


def shared_pool(world: World, M: int, seed: int = 0x5EED0006, margin: float = 1.0, tries: int = 32,
                standing_fraction: float = 0.2) -> np.ndarray:
    """pool [M,5]: the pedestrians of a shared world (BatchEpisode(shared=..., pool=...)) as people_msgs::Person rows x, y,
    vx, vy, vz. Each stands on a free cell of `world` (cost 0): the first of `tries` candidates, uniform over the floor at
    least `margin` from its border, that lies on one; without one, the centre of the free cell nearest the floor's centre.
    Speeds by make_scenes' law: standing_fraction of them stand, the others walk at 0.2 .. 1.2 m/s along a uniform heading;
    vz = 0. A pure function of its arguments through `uniform` (fields 1 .. 5, keyed by the person's index)."""
    ids = np.arange(int(M), dtype=np.int64)
    res, Hx, Hy = world.resolution, world.cells_x, world.cells_y
    x = world.origin[0] + margin + uniform(seed, ids, 1, tries) * (Hx * res - 2.0 * margin)    # [M,tries]
    y = world.origin[1] + margin + uniform(seed, ids, 2, tries) * (Hy * res - 2.0 * margin)
    ci = np.clip(np.floor((x - world.origin[0]) / res).astype(np.int64), 0, Hx - 1)
    cj = np.clip(np.floor((y - world.origin[1]) / res).astype(np.int64), 0, Hy - 1)
    ok = world.map[cj, ci] == 0
    jj, ii = np.meshgrid(np.arange(Hy), np.arange(Hx), indexing="ij")
    flat = int(np.argmin(np.where(world.map == 0, (ii + 0.5 - 0.5 * Hx) ** 2 + (jj + 0.5 - 0.5 * Hy) ** 2, np.inf)))
    pick = np.argmax(ok, axis=1)[:, None]
    px = np.where(ok.any(axis=1), np.take_along_axis(x, pick, 1)[:, 0], world.origin[0] + ((flat % Hx) + 0.5) * res)
    py = np.where(ok.any(axis=1), np.take_along_axis(y, pick, 1)[:, 0], world.origin[1] + ((flat // Hx) + 0.5) * res)
    heading = (uniform(seed, ids, 3)[:, 0] * 2.0 - 1.0) * np.pi
    standing = uniform(seed, ids, 4)[:, 0] < standing_fraction
    lv = np.where(standing, 0.0, 0.2 + uniform(seed, ids, 5)[:, 0])
    return np.ascontiguousarray(np.stack([px, py, lv * np.cos(heading), lv * np.sin(heading), np.zeros(int(M))], axis=1))


def pool_waypoints(world: World, pool: np.ndarray, K: int = 2, seed: int = 0x5EED0007, margin: float = 1.0, tries: int = 16):
    """Waypoint lists for the pedestrians of a shared world (BatchEpisode(pool_crowd=..., pool_waypoints=...,
    pool_n_waypoints=...)): (waypoints [M,K,2], n_waypoints [M]), a pure function of its arguments through `uniform` (keyed
    by the person's index), by crowd_waypoints' law on the world map. Every waypoint lies on the floor, at least `margin`
    from its border, on a free cell (cost 0). The first one lies straight ahead of the person's velocity, 0.5 .. 6 m away,
    so an episode starts the way the constant-velocity pool does; the others are anywhere on the floor. Each is the first
    of `tries` seeded candidates that qualifies (the first one falls back to the candidates of the others, all of them to
    the free cell nearest the floor's centre). A person that stands, or a row that is not finite, gets no waypoints: it
    stays where it is and only gives way."""
    pool = np.asarray(pool, np.float64).reshape(-1, 5)
    M, K = pool.shape[0], int(K)
    ids = np.arange(M, dtype=np.int64)
    res, Hx, Hy = float(world.resolution), world.cells_x, world.cells_y
    ox, oy = float(world.origin[0]), float(world.origin[1])

    def qualifies(x, y):                                                  # [M,tries] world points
        with np.errstate(invalid="ignore"):
            inside = (x >= ox + margin) & (x <= ox + Hx * res - margin) & (y >= oy + margin) & (y <= oy + Hy * res - margin)
            ci = np.clip(np.floor((np.where(inside, x, ox) - ox) / res).astype(np.int64), 0, Hx - 1)
            cj = np.clip(np.floor((np.where(inside, y, oy) - oy) / res).astype(np.int64), 0, Hy - 1)
        return inside & (world.map[cj, ci] == 0)

    def first_of(x, y, ok, fx, fy):                                       # the first qualifying candidate, else (fx, fy)
        pick = np.argmax(ok, axis=1)[:, None]
        any_ok = ok.any(axis=1)
        return (np.where(any_ok, np.take_along_axis(x, pick, 1)[:, 0], fx), np.where(any_ok, np.take_along_axis(y, pick, 1)[:, 0], fy))

    jj, ii = np.meshgrid(np.arange(Hy), np.arange(Hx), indexing="ij")
    flat = int(np.argmin(np.where(world.map == 0, (ii + 0.5 - 0.5 * Hx) ** 2 + (jj + 0.5 - 0.5 * Hy) ** 2, np.inf)))
    last_x, last_y = ox + ((flat % Hx) + 0.5) * res, oy + ((flat // Hx) + 0.5) * res
    wp = np.zeros((M, K, 2))
    anywhere = []
    for k in range(K):
        x = ox + margin + uniform(seed, ids, 200 + 2 * k, tries) * (Hx * res - 2.0 * margin)
        y = oy + margin + uniform(seed, ids, 201 + 2 * k, tries) * (Hy * res - 2.0 * margin)
        anywhere.append(first_of(x, y, qualifies(x, y), last_x, last_y))
    speed = np.hypot(pool[:, 2], pool[:, 3])
    walking = np.isfinite(pool[:, 0:4]).all(axis=1) & (speed > 0.0)
    yaw = np.arctan2(np.where(walking, pool[:, 3], 0.0), np.where(walking, pool[:, 2], 1.0))
    dist = 0.5 + 5.5 * uniform(seed, ids, 199, tries)
    x = np.where(walking, pool[:, 0], ox)[:, None] + dist * np.cos(yaw)[:, None]
    y = np.where(walking, pool[:, 1], oy)[:, None] + dist * np.sin(yaw)[:, None]
    if K > 0:
        wp[:, 0, 0], wp[:, 0, 1] = first_of(x, y, qualifies(x, y), *anywhere[0])
    for k in range(1, K):
        wp[:, k, 0], wp[:, k, 1] = anywhere[k]
    return np.ascontiguousarray(wp), np.ascontiguousarray(np.where(walking, K, 0).astype(np.int32))
