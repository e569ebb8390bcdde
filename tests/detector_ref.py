"""The yardstick of the people detector, written from include/smpc_detector.h alone: sequential, one robot at a time, Python
ints for Philox4x32-10 and the noise sums, numpy.float64 scalars for the arithmetic, every operation on its own. It shares
no code with the library or with the compiled rule."""
import numpy as np

F = np.float64
DETECTED, BODY_OCCLUDED, MISSED, NOT_FINITE = 0, 1, 2, 3
PURPOSE_MISS, PURPOSE_NOISE_X, PURPOSE_NOISE_Y, PURPOSE_CLUTTER = 0, 1, 2, 3
COUNTERS = ("detected", "body_occluded", "missed", "not_finite", "clutter", "persons_truncated", "clutter_truncated", "pose_not_finite")
M32 = 0xFFFFFFFF


def philox(counter, key):
    """Philox4x32-10: the four words of `counter` under the two words of `key`."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def thresholds(p_miss, p_clutter):
    return tuple(min(int(np.floor(F(v) * F(2.0 ** 32) + F(0.5))), 2 ** 32 - 1) for v in (p_miss, p_clutter))


def params(body_radius=0.25, p_miss=0.1, sigma=0.03, sigma_growth=0.002, clutter_candidates=2, p_clutter=0.05, clutter_range=5.0, seed=0,
           Nd=8, miss_threshold=None, clutter_threshold=None):
    """The call's scalars, formed as the caller of the library forms them."""
    miss, clutter = thresholds(p_miss, p_clutter)
    return dict(body_radius=F(body_radius), noise_scale=F(sigma) * np.sqrt(F(3.0)) / F(2.0 ** 32),
                noise_growth=F(sigma_growth) * np.sqrt(F(3.0)) / F(2.0 ** 32), clutter_scale=F(clutter_range) / F(2.0 ** 31),
                miss_threshold=miss if miss_threshold is None else int(miss_threshold),
                clutter_threshold=clutter if clutter_threshold is None else int(clutter_threshold),
                seed_lo=int(seed) & M32, seed_hi=int(seed) >> 32, Kc=int(clutter_candidates), Nd=int(Nd),
                given=dict(body_radius=body_radius, p_miss=p_miss, sigma=sigma, sigma_growth=sigma_growth, clutter_candidates=clutter_candidates,
                           p_clutter=p_clutter, clutter_range=clutter_range, seed=seed))


def draw(p, t, s, i, purpose):
    return philox((t, s, i, purpose), (p["seed_lo"], p["seed_hi"]))


def noise_sum(words):
    return sum(words) - (2 ** 33 - 2)


def occludes(dx, dy, dd, ex, ey, r2):
    """Does a person at offset e hide the person at offset d? e may be arrays (one answer each); a comparison with a NaN is
    false. numpy multiplies, adds and subtracts one operation at a time, each rounded on its own."""
    tk = ex * dx + ey * dy
    cr = ex * dy - ey * dx
    return (tk > 0.0) & (tk < dd) & (cr * cr <= r2 * dd)


def step_robot(state, people, count, pose, p, det, source, outcome):
    """One robot. state (s, t); people [Np][5]; det [Nd][5], source [Nd] and outcome [Np] as before the call (the rows the
    rule does not write keep their values). Returns ((s, t + 1), det_count, counters)."""
    s, t = int(state[0]), int(state[1])
    Np, Nd, Kc = len(people), p["Nd"], p["Kc"]
    n = min(max(int(count), 0), Np)
    c = dict.fromkeys(COUNTERS, 0)
    new_state = (s, (t + 1) & M32)
    with np.errstate(all="ignore"):
        rx, ry = F(pose[0]), F(pose[1])
        if not (np.isfinite(rx) and np.isfinite(ry)):                                     # 1: the robot itself
            outcome[:n] = NOT_FINITE
            c["pose_not_finite"] = 1
            return new_state, 0, c
        usable, off = [], {}
        for j in range(n):
            px, py = F(people[j][0]), F(people[j][1])
            if np.isfinite(px) and np.isfinite(py):
                dx, dy = px - rx, py - ry
                off[j] = (dx, dy, dx * dx + dy * dy)
                usable.append(j)
            else:
                outcome[j] = NOT_FINITE
                c["not_finite"] += 1
        r2 = p["body_radius"] * p["body_radius"]
        ex, ey = np.array([off[k][0] for k in usable], np.float64), np.array([off[k][1] for k in usable], np.float64)
        rows = []                                                                         # (source, row of five doubles)
        for at, j in enumerate(usable):
            dx, dy, dd = off[j]
            others = np.arange(len(usable)) != at
            if p["body_radius"] > 0.0 and bool((occludes(dx, dy, dd, ex, ey, r2) & others).any()):                          # 2
                outcome[j] = BODY_OCCLUDED
                c["body_occluded"] += 1
                continue
            if draw(p, t, s, j, PURPOSE_MISS)[0] < p["miss_threshold"]:                   # 3
                outcome[j] = MISSED
                c["missed"] += 1
                continue
            outcome[j] = DETECTED
            c["detected"] += 1
            row = np.array(people[j], np.float64)
            scale = p["noise_scale"] + p["noise_growth"] * dd                             # 4
            if scale != 0.0:
                sx, sy = noise_sum(draw(p, t, s, j, PURPOSE_NOISE_X)), noise_sum(draw(p, t, s, j, PURPOSE_NOISE_Y))
                row[0] = F(people[j][0]) + F(sx) * scale
                row[1] = F(people[j][1]) + F(sy) * scale
            rows.append((j, row))
        n_persons = len(rows)
        for k in range(Kc):                                                               # 5
            w = draw(p, t, s, k, PURPOSE_CLUTTER)
            if w[0] < p["clutter_threshold"]:
                signed = lambda v: v - 2 ** 32 if v >= 2 ** 31 else v
                rows.append((-1 - k, np.array([rx + F(signed(w[1])) * p["clutter_scale"], ry + F(signed(w[2])) * p["clutter_scale"], 0.0, 0.0, 0.0])))
                c["clutter"] += 1
        det_count = min(Nd, len(rows))                                                    # 6
        for r in range(det_count):
            source[r] = rows[r][0]
            det[r] = rows[r][1]
        c["persons_truncated"] = max(0, n_persons - Nd)
        c["clutter_truncated"] = len(rows) - det_count - c["persons_truncated"]
    return new_state, det_count, c


def step(draw_state, people, count, pose, p, det=None, source=None, outcome=None):
    """One tick of a batch: draw_state [B,2] uint32, people [B,Np,5], count [B], pose [B,3]; det [B,Nd,5] / source [B,Nd] /
    outcome [B,Np] as before the call (default NaN / -99 / 255). Returns (new draw_state, (det, det_count, source, outcome),
    counters: name -> [B])."""
    people = np.asarray(people, np.float64)
    B, Np, Nd = people.shape[0], people.shape[1], p["Nd"]
    det = np.full((B, Nd, 5), np.nan) if det is None else np.array(det, np.float64)
    source = np.full((B, Nd), -99, np.int32) if source is None else np.array(source, np.int32)
    outcome = np.full((B, Np), 255, np.uint8) if outcome is None else np.array(outcome, np.uint8)
    new = np.array(draw_state, np.uint32)
    det_count = np.zeros(B, np.int32)
    counters = {k: np.zeros(B, np.int64) for k in COUNTERS}
    for b in range(B):
        (s, t), det_count[b], c = step_robot(new[b], people[b], count[b], pose[b], p, det[b], source[b], outcome[b])
        new[b] = (s, t)
        for k in COUNTERS:
            counters[k][b] = c[k]
    return new, (det, det_count, source, outcome), counters
