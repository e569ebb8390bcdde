"""The yardstick of the people tracker, written from include/smpc_tracker.h alone: sequential, over plain Python lists with
numpy.float64 scalars, every operation on its own. All qualifying pairs are sorted by (d2, i, j) and accepted greedily. It
shares no code with the library or with the compiled rule."""
import numpy as np

F = np.float64
FREE, TENTATIVE, CONFIRMED = 0, 1, 2
COUNTERS = ("matched", "coasted", "freed_by_misses", "tentative_freed", "born", "dropped", "newly_confirmed", "sanitised", "ties")


def params(alpha=0.5, beta=0.2, gate=0.6, confirm_hits=3, max_missed=20, slots=16, dt=0.1, Np=None):
    """The call's scalars: gain = beta / dt is formed here, as the caller of the library forms it."""
    return dict(alpha=F(alpha), beta=F(beta), gain=F(beta) / F(dt), gate=F(gate), confirm_hits=int(confirm_hits), max_missed=int(max_missed),
                Nt=int(slots), dt=F(dt), Np=int(slots if Np is None else Np))


def zero_state(B, Nt):
    return np.zeros((B, Nt, 4)), np.zeros((B, Nt, 4), np.int32), np.zeros(B, np.int32)


def _wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def bits(v):
    return int(np.array(v, np.float64).view(np.uint64))


def step_robot(tracks, meta, next_id, det, count, pose, p, people, source):
    """One robot. tracks [Nt][4], meta [Nt][4], det [Nd][>=2] rows, people [Np][5] and source [Np][2] as before the call
    (rows from the returned count on keep their values). Returns (tracks, meta, next_id, people, count, source, counters)."""
    Nt, Np, Nd = p["Nt"], p["Np"], len(det)
    dt, alpha, gain, gate = p["dt"], p["alpha"], p["gain"], p["gate"]
    n = dict.fromkeys(COUNTERS, 0)
    slots = []
    with np.errstate(all="ignore"):
        for i in range(Nt):                                                               # 0: sanitise
            x, y, vx, vy = (F(v) for v in tracks[i])
            state, hits, missed, tid = (int(v) for v in meta[i])
            if state not in (TENTATIVE, CONFIRMED) or not all(np.isfinite(v) for v in (x, y, vx, vy)):
                if state != 0 or hits != 0 or missed != 0 or tid != 0 or any(bits(v) != 0 for v in (x, y, vx, vy)):
                    n["sanitised"] += 1
                slots.append(None)
                continue
            slots.append(dict(x=x, y=y, vx=vx, vy=vy, state=state, hits=hits, missed=missed, id=tid,
                              xp=x + vx * dt, yp=y + vy * dt, match=None))                # 1: predict
        cnt = min(max(int(count), 0), Nd)                                                 # 2: detections
        used = [j for j in range(cnt) if np.isfinite(det[j][0]) and np.isfinite(det[j][1])]
        g2 = gate * gate                                                                  # 3: associate
        pairs = []
        for i, sl in enumerate(slots):
            if sl is None:
                continue
            for j in used:
                rx, ry = F(det[j][0]) - sl["xp"], F(det[j][1]) - sl["yp"]
                d2 = rx * rx + ry * ry
                if d2 <= g2:
                    pairs.append((float(d2), i, j, rx, ry))
        pairs.sort(key=lambda q: q[:3])
        taken = set()
        for k, (d2, i, j, rx, ry) in enumerate(pairs):
            if slots[i]["match"] is None and j not in taken:
                # an exact tie of d2 that the indices resolve: a later pair of the same d2 competes for this slot or detection
                if any(q[0] == d2 and (q[1] == i or q[2] == j) and slots[q[1]]["match"] is None and q[2] not in taken
                       for q in pairs[k + 1:]):
                    n["ties"] += 1
                slots[i]["match"] = (j, rx, ry)
                taken.add(j)
        for i, sl in enumerate(slots):
            if sl is None:
                continue
            if sl["match"] is not None:                                                   # 4: update
                _, rx, ry = sl["match"]
                sl["x"], sl["y"] = sl["xp"] + alpha * rx, sl["yp"] + alpha * ry
                sl["vx"], sl["vy"] = sl["vx"] + gain * rx, sl["vy"] + gain * ry
                sl["hits"], sl["missed"] = min(sl["hits"] + 1, 2 ** 30), 0
                n["matched"] += 1
                if sl["state"] == TENTATIVE and sl["hits"] >= p["confirm_hits"]:
                    sl["state"] = CONFIRMED
                    n["newly_confirmed"] += 1
            else:                                                                         # 5: coast
                sl["x"], sl["y"], sl["missed"] = sl["xp"], sl["yp"], _wrap32(sl["missed"] + 1)
                if sl["state"] == TENTATIVE:
                    slots[i] = None
                    n["tentative_freed"] += 1
                elif sl["missed"] > p["max_missed"]:
                    slots[i] = None
                    n["freed_by_misses"] += 1
                else:
                    n["coasted"] += 1
        next_id = int(next_id)
        for j in used:                                                                    # 6: birth
            if j in taken:
                continue
            free = [i for i in range(Nt) if slots[i] is None]
            if not free:
                n["dropped"] += 1
                continue
            slots[free[0]] = dict(x=F(det[j][0]), y=F(det[j][1]), vx=F(0.0), vy=F(0.0), hits=1, missed=0, id=_wrap32(next_id),
                                  state=CONFIRMED if p["confirm_hits"] <= 1 else TENTATIVE)
            next_id = (next_id + 1) % 2 ** 32
            n["born"] += 1
        new_tracks = [[F(0.0)] * 4 if sl is None else [sl["x"], sl["y"], sl["vx"], sl["vy"]] for sl in slots]
        new_meta = [[0] * 4 if sl is None else [sl["state"], sl["hits"], sl["missed"], sl["id"]] for sl in slots]
        people, source = [list(r) for r in people], [list(r) for r in source]             # 7: output
        if not (np.isfinite(pose[0]) and np.isfinite(pose[1])):
            return new_tracks, new_meta, _wrap32(next_id), people, 0, source, n
        order = []
        for i, sl in enumerate(slots):
            if sl is not None and sl["state"] == CONFIRMED:
                ddx, ddy = sl["x"] - F(pose[0]), sl["y"] - F(pose[1])
                dr2 = ddx * ddx + ddy * ddy
                order.append((bits(dr2) if np.isfinite(dr2) else 2 ** 64 - 1, i))
        order.sort()
        out = min(Np, len(order))
        for r, (_, i) in enumerate(order[:out]):
            sl = slots[i]
            people[r] = [sl["x"], sl["y"], sl["vx"], sl["vy"], F(0.0)]
            source[r] = [i, sl["id"]]
    return new_tracks, new_meta, _wrap32(next_id), people, out, source, n


def step(state, detections, count, pose, p, people=None, source=None):
    """One call for B robots. state = (tracks [B,Nt,4], track_meta [B,Nt,4] int32, next_id [B] int32); detections [B,Nd,5],
    count [B], pose [B,3]. people [B,Np,5] / source [B,Np,2]: the arrays before the call (default NaN / -1). Returns
    (new state, (people, count, source), counters: name -> [B] int)."""
    tracks, meta, next_id = state
    detections = np.asarray(detections, np.float64)
    B, Nt, Np = detections.shape[0], p["Nt"], p["Np"]
    assert np.shape(tracks) == (B, Nt, 4) and np.shape(meta) == (B, Nt, 4) and np.shape(next_id) == (B,)
    people = np.full((B, Np, 5), np.nan) if people is None else np.array(people, np.float64)
    source = np.full((B, Np, 2), -1, np.int32) if source is None else np.array(source, np.int32)
    new_t, new_m, new_n = np.zeros((B, Nt, 4)), np.zeros((B, Nt, 4), np.int32), np.zeros(B, np.int32)
    out_count, counters = np.zeros(B, np.int32), {k: np.zeros(B, np.int64) for k in COUNTERS}
    for b in range(B):
        t, m, nid, ppl, c, src, n = step_robot(tracks[b], meta[b], next_id[b], detections[b], count[b], pose[b], p, people[b], source[b])
        new_t[b], new_m[b], new_n[b], people[b], out_count[b], source[b] = np.array(t, np.float64), m, nid, np.array(ppl, np.float64), c, src
        for k in COUNTERS:
            counters[k][b] = n[k]
    return (new_t, new_m, new_n), (people, out_count, source), counters
