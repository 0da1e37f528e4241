"""Numpy models of the rival row of the device step (include/ftgp.h: FTGP_RIVAL_FIXED, ftgp_device_io_rivals).

`rival_rows64` / `rival_rows` restate the header's text operation by operation: binary64 elementwise numpy (one rounding per
operation, nothing fused), the same expressions in the same order, the same comparisons.  They take rows of ftgp_get_pose,
column 3 and 4 of ftgp_get_progress and ftgp_get_race_steps' finish steps; the per-car search is tests/frame_model.py's.
`place_term` / `place_reward` restate the place reward.

`independent_rows` is independent of that text: the mates rotated by -yaw with np.cos / np.sin of arctan2-derived angles, sorted with
np.argsort(kind="stable") on np.hypot, the places from sorting a key tuple.
"""
import numpy as np

from tests import frame_model as fm

RIVAL_FIXED = 4
RIVAL_FLOATS = 8
MAX_RIVALS = 7
PLACE, N_RACING, GAP_AHEAD, GAP_BEHIND = range(4)
FWD, LEFT, COS_REL, SIN_REL, V_FWD, V_LEFT, TRACK_GAP, PRESENT = range(8)


def _wrap(v):
    v = np.where(v >= 50.0, v - 100.0, v)
    return np.where(v < -50.0, v + 100.0, v)


def progress64(path, pose, abs_completion):
    """Step 1: (g, s, c, off) of every car."""
    _, s, off, _, c = fm.frame_rows64(path, pose)
    f = _wrap(s - c.astype(np.float64))
    f = np.where(off, 0.0, f)
    return np.asarray(abs_completion).astype(np.float64) + f, s, c, off


def _rows_from(g, s, pose, finished, finish_step, cpe, n_rivals):
    pose = np.asarray(pose, dtype=np.float64)
    n = len(pose)
    assert n % cpe == 0 and 0 <= n_rivals <= MAX_RIVALS
    E = n // cpe
    env = lambda v: np.asarray(v).reshape(E, cpe)
    g, s = env(g), env(s)
    fin, fs = env(finished) != 0, env(finish_step).astype(np.int64)
    x, y, qw, qz, vx, vy = (env(pose[:, k]) for k in (0, 1, 3, 6, 7, 8))
    ch, sh = qw * qw - qz * qz, 2.0 * (qw * qz)
    slot = np.arange(cpe)
    # [E, a, b]: b's value along the last axis, a's along the middle one
    A, B = (lambda v: v[:, :, None]), (lambda v: v[:, None, :])
    a_idx, b_idx = slot[None, :, None], slot[None, None, :]
    other = a_idx != b_idx
    with np.errstate(invalid="ignore"):
        both = B(fin) & A(fin) & ((B(fs) < A(fs)) | ((B(fs) == A(fs)) & (b_idx < a_idx)))
        racing = ~B(fin) & ~A(fin) & ((B(g) > A(g)) | ((B(g) == A(g)) & (b_idx < a_idx)))
    ahead = other & (both | (B(fin) & ~A(fin)) | racing)
    place = 1 + ahead.sum(axis=2)
    n_racing = np.broadcast_to((~fin).sum(axis=1)[:, None], (E, cpe))
    mate = other & ~B(fin) & ~A(fin)
    gap = B(g) - A(g)
    gap_ahead = np.where(mate & ahead, gap, np.inf).min(axis=2)
    gap_behind = np.where(mate & ~ahead, A(g) - B(g), np.inf).min(axis=2)
    rows = np.zeros((E, cpe, RIVAL_FIXED + RIVAL_FLOATS * n_rivals))
    rows[:, :, PLACE], rows[:, :, N_RACING] = place, n_racing
    rows[:, :, GAP_AHEAD] = np.where(np.isinf(gap_ahead), 0.0, gap_ahead)
    rows[:, :, GAP_BEHIND] = np.where(np.isinf(gap_behind), 0.0, gap_behind)
    dx, dy = B(x) - A(x), B(y) - A(y)
    d2 = dx * dx + dy * dy
    order = np.argsort(np.where(mate, d2, np.inf), axis=2, kind="stable")         # ascending, on equal d2 the smaller slot first
    n_mates = mate.sum(axis=2)
    dvx, dvy = B(vx) - A(vx), B(vy) - A(vy)
    entries = np.stack([dx * A(ch) + dy * A(sh), dy * A(ch) - dx * A(sh), B(ch) * A(ch) + B(sh) * A(sh), B(sh) * A(ch) - B(ch) * A(sh),
                        dvx * A(ch) + dvy * A(sh), dvy * A(ch) - dvx * A(sh), _wrap(B(s) - A(s)), np.ones_like(dx)], axis=3)
    mates = np.full((E, cpe, MAX_RIVALS), -1, dtype=np.int64)
    for k in range(MAX_RIVALS):
        if k >= cpe:
            break
        b = order[:, :, k]
        have = k < n_mates
        mates[:, :, k] = np.where(have, b, -1)
        if k < n_rivals:
            e = np.take_along_axis(entries, b[:, :, None, None], axis=2)[:, :, 0]
            rows[:, :, RIVAL_FIXED + RIVAL_FLOATS * k: RIVAL_FIXED + RIVAL_FLOATS * (k + 1)] = np.where(have[:, :, None], e, 0.0)
    return rows.reshape(n, -1), g.reshape(n), place.reshape(n), mates.reshape(n, MAX_RIVALS)


def rival_rows64(path, pose, abs_completion, finished, finish_step, cpe, n_rivals):
    """The header's row before the rounding to binary32: (rows float64 [n, 4 + 8 n_rivals], g [n], place [n], mates [n, 7] = the slots
    of every car's mates in their order, -1 behind the last)."""
    g, s, _, _ = progress64(np.asarray(path, dtype=np.float64), np.asarray(pose, dtype=np.float64), abs_completion)
    return _rows_from(g, s, pose, finished, finish_step, cpe, n_rivals)


def rival_rows(path, pose, abs_completion, finished, finish_step, cpe, n_rivals):
    """The row as the library writes it: every entry rounded once to binary32."""
    return rival_rows64(path, pose, abs_completion, finished, finish_step, cpe, n_rivals)[0].astype(np.float32)


def rival_rows_blocks(paths, envs_per_track, cpe, pose, abs_completion, finished, finish_step, n_rivals):
    """rival_rows64 on a multi-track handle (env block t = envs_per_track[t] consecutive envs on paths[t]): (rows float32, g, place)."""
    pose = np.asarray(pose, dtype=np.float64)
    n = len(pose)
    rows, g, place = np.empty((n, RIVAL_FIXED + RIVAL_FLOATS * n_rivals), dtype=np.float32), np.empty(n), np.empty(n, dtype=np.int64)
    first = 0
    for t, m in enumerate(envs_per_track):
        k = slice(first, first + m * cpe)
        r, g[k], place[k], _ = rival_rows64(paths[t], pose[k], np.asarray(abs_completion)[k], np.asarray(finished)[k],
                                            np.asarray(finish_step)[k], cpe, n_rivals)
        rows[k] = r.astype(np.float32)
        first += m * cpe
    assert first == n
    return rows, g, place


def place_term(w, p0, p1, finished0):
    """The place term: float32 w times the float32 of the places gained, nothing for a car that had finished when the call began."""
    gained = np.where(np.asarray(finished0, dtype=bool), 0, np.asarray(p0, dtype=np.int64) - np.asarray(p1, dtype=np.int64))
    return (np.float32(w) * gained.astype(np.float32)).astype(np.float32)


def place_reward(reward, w, p0, p1, finished0):
    """The reward behind the penalties with the place term on it: one binary32 multiplication, one binary32 addition; with w == 0 the
    reward itself."""
    if w == 0:
        return reward
    return (np.asarray(reward, dtype=np.float32) + place_term(w, p0, p1, finished0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------- independent
def independent_rows(path, pose, abs_completion, finished, finish_step, cpe, n_rivals):
    """Independent of the header's operations: per env, a python loop.  Race progress from the brute-force polyline position of
    `frame_model.polyline_frame` on the two segments around the nearest point; places by sorting key tuples; mates by a stable argsort
    on np.hypot, rotated by -yaw with np.cos / np.sin.  Returns (rows float64, place, mates) like `rival_rows64`."""
    path, pose = np.asarray(path, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    n = len(pose)
    dist, _, _, s_all, yaw = fm.polyline_frame(path, pose)
    c = np.hypot(path[None, :, 0] - pose[:, None, 0], path[None, :, 1] - pose[:, None, 1]).argmin(axis=1)
    off = np.hypot(path[c, 0] - pose[:, 0], path[c, 1] - pose[:, 1]) > 1.0
    idx = np.arange(n)
    prev = (c + 99) % 100
    seg = np.where(dist[idx, prev] < dist[idx, c], prev, c)
    s = s_all[idx, seg] % 100.0
    f = (s - c + 50.0) % 100.0 - 50.0
    g = np.asarray(abs_completion, dtype=np.float64) + np.where(off, 0.0, f)
    fin, fs = np.asarray(finished) != 0, np.asarray(finish_step)
    rows = np.zeros((n, RIVAL_FIXED + RIVAL_FLOATS * n_rivals))
    place, mates = np.zeros(n, dtype=np.int64), np.full((n, MAX_RIVALS), -1, dtype=np.int64)
    for e0 in range(0, n, cpe):
        cars = list(range(e0, e0 + cpe))
        # finishers first in (finish_step, slot) order, then the racing cars by falling g, the smaller slot first on equal g
        ranking = sorted(cars, key=lambda k: (0, int(fs[k]), k, 0) if fin[k] else (1, -g[k], k, 0))
        racing = [k for k in ranking if not fin[k]]
        for a in cars:
            place[a] = ranking.index(a) + 1
            rows[a, PLACE], rows[a, N_RACING] = place[a], len(racing)
            if fin[a]:
                continue
            i = racing.index(a)
            rows[a, GAP_AHEAD] = g[racing[i - 1]] - g[a] if i > 0 else 0.0
            rows[a, GAP_BEHIND] = g[a] - g[racing[i + 1]] if i + 1 < len(racing) else 0.0
            others = np.array([k for k in cars if k != a and not fin[k]], dtype=np.int64)
            if not len(others):
                continue
            rel = pose[others, 0:2] - pose[a, 0:2]
            near = others[np.argsort(np.hypot(rel[:, 0], rel[:, 1]), kind="stable")]
            mates[a, :len(near)] = near - e0
            co, si = np.cos(-yaw[a]), np.sin(-yaw[a])
            for k, b in enumerate(near[:n_rivals]):
                d, dv, rel_yaw = pose[b, 0:2] - pose[a, 0:2], pose[b, 7:9] - pose[a, 7:9], yaw[b] - yaw[a]
                rows[a, RIVAL_FIXED + RIVAL_FLOATS * k: RIVAL_FIXED + RIVAL_FLOATS * (k + 1)] = [
                    co * d[0] - si * d[1], si * d[0] + co * d[1], np.cos(rel_yaw), np.sin(rel_yaw),
                    co * dv[0] - si * dv[1], si * dv[0] + co * dv[1], (s[b] - s[a] + 50.0) % 100.0 - 50.0, 1.0]
    return rows, place, mates


# ---------------------------------------------------------------------------------------------------------------------- hand-written envs
EAST, WEST = (1.0, 0.0), (0.0, 1.0)          # (qw, qz) of yaw 0 and yaw pi, exact


def hand_scenes():
    """Envs on `frame_model.square_path()` whose rows are exact: name -> cars (x, y, (qw, qz), vx, vy, absolute_completion, finished,
    finish_step).  (3.25, 0) lies between points 6 and 7: c = 6, s = 6.5; (0, 0.25) between points 99 and 0: c = 0, s = 99.5."""
    return {
        "alone": [(3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0)],
        "ahead and behind": [(3.25, 0.0, EAST, 1.0, 0.0, 6, 0, 0), (5.25, 0.0, EAST, 1.5, 0.25, 10, 0, 0)],
        "left, looking west, equal g": [(3.25, 0.25, WEST, 0.0, 0.0, 6, 0, 0), (3.25, -0.25, EAST, 2.0, 1.0, 6, 0, 0)],
        "equal d2": [(2.25, 0.0, EAST, 0.0, 0.0, 4, 0, 0), (3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0), (4.25, 0.0, EAST, 0.0, 0.0, 8, 0, 0)],
        "one spot": [(3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0), (3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0)],
        "across the line": [(0.0, 0.25, EAST, 0.0, 0.0, 100, 0, 0), (0.125, 0.0, EAST, 0.0, 0.0, 100, 0, 0)],
        "half a lap apart": [(5.0, 0.0, EAST, 0.0, 0.0, 10, 0, 0), (7.5, 12.5, EAST, 0.0, 0.0, 60, 0, 0)],
        "off-track mate": [(3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0), (3.25, -2.0, EAST, 0.0, 0.0, 6, 0, 0)],
        "finishers": [(3.25, 0.0, EAST, 0.0, 0.0, 6, 0, 0), (4.25, 0.0, EAST, 0.0, 0.0, 100, 1, 100), (2.25, 0.0, EAST, 0.0, 0.0, 4, 0, 0),
                      (6.25, 0.0, EAST, 0.0, 0.0, 100, 1, 100), (8.25, 0.0, EAST, 0.0, 0.0, 100, 1, 90)],
    }


def scene_arrays(cars):
    """cars of `hand_scenes` -> (pose rows of ftgp_get_pose, absolute_completion, finished, finish_step)."""
    pose = np.zeros((len(cars), 13))
    for k, (x, y, q, vx, vy, _, _, _) in enumerate(cars):
        pose[k, 0], pose[k, 1], pose[k, 3], pose[k, 6], pose[k, 7], pose[k, 8] = x, y, q[0], q[1], vx, vy
    return (pose, np.array([c[5] for c in cars], dtype=np.int32), np.array([c[6] for c in cars], dtype=np.int32),
            np.array([c[7] for c in cars], dtype=np.int64))
