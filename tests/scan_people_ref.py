"""The yardstick of the scan-based people detector, written from the rule in include/smpc_scan_people.h alone: one robot after
another, one beam after another, plain Python integers for everything about cells and numpy float64 for the position (one
rounding per operation; numpy's division and square root are correctly rounded). Nothing here knows how the kernel walks."""
import numpy as np

KIND_NONE, KIND_WORLD, KIND_AGENT, KIND_CORNER_PAIR, KIND_INVALID, KIND_NO_ROBOT = 0, 1, 2, 3, 4, 5

F = np.float64


def params(link_d2, min_points, width_d2_min, width_d2_max, range_d2, subtract_map=1, body_offset=0.0, res=0.125, origin=(0.0, 0.0)):
    return dict(link_d2=int(link_d2), min_points=int(min_points), width_d2_min=int(width_d2_min), width_d2_max=int(width_d2_max),
                range_d2=int(range_d2), subtract_map=int(subtract_map), body_offset=float(body_offset), res=float(res),
                origin=(float(origin[0]), float(origin[1])))


def robot_cell(x, y, origin, res):
    """Rule 1 (smpc_sensed_costmap.h rule 1): the cell, or None."""
    x, y = F(x), F(y)
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    with np.errstate(all="ignore"):
        q = [np.floor((p - F(o)) / F(res)) for p, o in ((x, origin[0]), (y, origin[1]))]
    if not all(abs(v) <= 2.0 ** 30 for v in q):      # false for a NaN
        return None
    return int(q[0]), int(q[1])


def segments(p, kind, cell):
    """Rules 2 to 5 for one robot: [(s, m, Sx, Sy, chord)] in ascending s, and (wrapped, whole_circle)."""
    n = len(kind)
    o = [(int(cx), int(cy)) for cx, cy in cell]
    fg = [(int(k) in (KIND_AGENT, KIND_CORNER_PAIR) or (int(k) == KIND_WORLD and p["subtract_map"] == 0))
          and ox * ox + oy * oy <= p["range_d2"] for k, (ox, oy) in zip(kind, o)]
    linked = [False] * n
    if n >= 2:
        for k in range(n):
            q = (k - 1 + n) % n
            linked[k] = fg[k] and fg[q] and (o[k][0] - o[q][0]) ** 2 + (o[k][1] - o[q][1]) ** 2 <= p["link_d2"]
    starts = [k for k in range(n) if fg[k] and not linked[k]]
    runs = []
    for s in starts:
        m = 1
        while linked[(s + m) % n]:      # a start is not linked, so the walk ends at the next start at the latest
            m += 1
        runs.append((s, m))
    whole = any(fg) and not starts
    if whole:
        runs = [(0, n)]
    out, wrapped = [], 0
    for s, m in runs:
        ks = [(s + i) % n for i in range(m)]
        first, last = o[ks[0]], o[ks[-1]]
        out.append((s, m, sum(o[k][0] for k in ks), sum(o[k][1] for k in ks), (first[0] - last[0]) ** 2 + (first[1] - last[1]) ** 2))
        wrapped += s + m > n
    return out, wrapped, whole


def gate(p, m, chord):
    """Rule 6: 0 accepted, 1 rejected by points, 2 rejected by width."""
    if m < p["min_points"]:
        return 1
    if chord < p["width_d2_min"] or chord > p["width_d2_max"]:
        return 2
    return 0


def position(p, a, pose, m, Sx, Sy):
    """Rule 7: (px, py, d == 0)."""
    res, off = F(p["res"]), F(p["body_offset"])
    with np.errstate(all="ignore"):
        c = [F(p["origin"][i]) + ((F(a[i]) + F(S) / F(m)) + F(0.5)) * res for i, S in enumerate((Sx, Sy))]
        r = [c[0] - F(pose[0]), c[1] - F(pose[1])]
        d = np.sqrt(r[0] * r[0] + r[1] * r[1])
        if off > 0.0 and np.isfinite(d) and d > 0.0:
            k = off / d
            return c[0] + r[0] * k, c[1] + r[1] * k, False
    return c[0], c[1], bool(d == 0.0)


def run(p, Nd, pose, kind, cell, detections=None, det_segment=None):
    """All robots. detections [B,Nd,5] / det_segment [B,Nd,4]: the arrays before the call (default NaN / -99); rows from
    det_count on keep them. Returns the four outputs plus `counters` (what the cases exercise) and per robot `accepted`."""
    pose, kind, cell = np.asarray(pose, np.float64), np.asarray(kind, np.uint8), np.asarray(cell, np.int32)
    B, n = kind.shape
    det = np.full((B, Nd, 5), np.nan) if detections is None else np.array(detections, np.float64)
    seg = np.full((B, Nd, 4), -99, np.int32) if det_segment is None else np.array(det_segment, np.int32)
    count, stats = np.zeros(B, np.int32), np.zeros((B, 4), np.int32)
    counters = dict(wrapped=0, crossing=0, whole_circle=0, dropped=0, d_zero=0, no_cell=0)
    for b in range(B):
        a = robot_cell(pose[b, 0], pose[b, 1], p["origin"], p["res"])
        if a is None:
            counters["no_cell"] += 1
            continue
        segs, wrapped, whole = segments(p, kind[b], cell[b])
        counters["wrapped"] += wrapped
        counters["whole_circle"] += whole
        for s, m, Sx, Sy, chord in segs:
            counters["crossing"] += (s // 64) != ((s + m - 1) // 64)
            g = gate(p, m, chord)
            stats[b, 0] += 1
            stats[b, g if g else 3] += 1
            if g:
                continue
            if count[b] == Nd:
                counters["dropped"] += 1
                continue
            px, py, zero = position(p, a, pose[b], m, Sx, Sy)
            counters["d_zero"] += zero
            det[b, count[b]] = (px, py, 0.0, 0.0, 0.0)
            seg[b, count[b]] = (s, m, Sx, Sy)
            count[b] += 1
    return dict(detections=det, det_count=count, det_segment=seg, seg_stats=stats, counters=counters)


def same(got, want, keys=("detections", "det_count", "det_segment", "seg_stats")):
    """Bit for bit, NaN prefill included; a key whose `got` is None is skipped."""
    return all(got[k] is None or (got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes())
               for k in keys)
