"""Numpy models of the track-frame row of the device step (include/ftgp.h: FTGP_FRAME_FIXED, ftgp_device_io_frame).

`frame_rows64` / `frame_rows` restate the header's text operation by operation: binary64 elementwise numpy (one rounding per
operation, nothing fused), the same expressions in the same order, the same comparisons.  They take rows of ftgp_get_pose.
`dense_reward` restates the dense progress reward, `penalised` the order of the penalties.

`polyline_frame` is independent of that text: brute force over all 100 segments of the closed polyline with np.hypot, the tangent as
an angle (arctan2, cos, sin), the yaw as 2 atan2(qz, qw).
"""
import numpy as np

PATH_POINTS = 100
FRAME_FIXED = 4
MAX_LOOKAHEAD = 16
LAT, COS_H, SIN_H, S_NORM = range(4)


def _segment(path, a, x, y):
    """Step 2: the poses (x, y) projected on segments a -> a + 1 (arrays of equal length)."""
    b = (a + 1) % PATH_POINTS
    xa, ya = path[a, 0], path[a, 1]
    ex, ey = path[b, 0] - xa, path[b, 1] - ya
    L2 = ex * ex + ey * ey
    rx, ry = x - xa, y - ya
    flat = L2 == 0.0
    ex, ey, L2 = np.where(flat, 1.0, ex), np.where(flat, 0.0, ey), np.where(flat, 1.0, L2)
    t = (rx * ex + ry * ey) / L2
    t = np.where(flat, 0.0, np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t)))
    fx, fy = xa + t * ex, ya + t * ey
    gx, gy = x - fx, y - fy
    g2 = gx * gx + gy * gy
    return dict(a=a, ex=ex, ey=ey, L2=L2, rx=rx, ry=ry, t=t, g2=g2)


def frame_rows64(path, pose, n_ahead=0, stride=1):
    """The header's row before the rounding to binary32: (rows float64 [n, 4 + 2 n_ahead], s [n], off [n], a [n], c [n])."""
    path, pose = np.asarray(path, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    assert path.shape == (PATH_POINTS, 2) and 0 <= n_ahead <= MAX_LOOKAHEAD and 1 <= stride <= 50
    x, y, qw, qz = pose[:, 0], pose[:, 1], pose[:, 3], pose[:, 6]
    dx, dy = path[None, :, 0] - x[:, None], path[None, :, 1] - y[:, None]
    d = dx * dx + dy * dy
    c = np.argmin(d, axis=1)                                  # the first index of the smallest
    off = d[np.arange(len(c)), c] > 1.0
    A, B = _segment(path, (c + 99) % PATH_POINTS, x, y), _segment(path, c, x, y)
    take_a = A["g2"] < B["g2"]
    g = {k: np.where(take_a, A[k], B[k]) for k in A}
    a, ex, ey, rx, ry, t = g["a"], g["ex"], g["ey"], g["rx"], g["ry"], g["t"]
    ln = np.sqrt(g["L2"])
    ch, sh = qw * qw - qz * qz, 2.0 * (qw * qz)
    s = a.astype(np.float64) + t
    s = np.where(s >= 100.0, s - 100.0, s)
    rows = np.empty((len(x), FRAME_FIXED + 2 * n_ahead))
    rows[:, LAT] = (ex * ry - ey * rx) / ln
    rows[:, COS_H] = (ex * ch + ey * sh) / ln
    rows[:, SIN_H] = (ey * ch - ex * sh) / ln
    rows[:, S_NORM] = s / 100.0
    for k in range(n_ahead):
        q = (a + 1 + k * stride) % PATH_POINTS
        dx, dy = path[q, 0] - x, path[q, 1] - y
        rows[:, 4 + 2 * k] = dx * ch + dy * sh
        rows[:, 5 + 2 * k] = dy * ch - dx * sh
    return rows, s, off, a, c


def frame_rows(path, pose, n_ahead=0, stride=1):
    """The row as the library writes it: every entry rounded once to binary32."""
    return frame_rows64(path, pose, n_ahead, stride)[0].astype(np.float32)


def env_paths(paths, envs_per_track, cpe):
    """The path of every car of a multi-track handle: env block t = envs_per_track[t] consecutive envs on paths[t]."""
    return [paths[t] for t, n in enumerate(envs_per_track) for _ in range(n * cpe)]


def frame_blocks(paths, envs_per_track, cpe, pose, n_ahead=0, stride=1):
    """frame_rows64 on a multi-track handle: (rows float32, s, off)."""
    pose = np.asarray(pose, dtype=np.float64)
    rows, s, off = np.empty((len(pose), FRAME_FIXED + 2 * n_ahead), dtype=np.float32), np.empty(len(pose)), np.empty(len(pose), dtype=bool)
    first = 0
    for t, n in enumerate(envs_per_track):
        k = slice(first, first + n * cpe)
        r, s[k], off[k], _, _ = frame_rows64(paths[t], pose[k], n_ahead, stride)
        rows[k] = r.astype(np.float32)
        first += n * cpe
    assert first == len(pose)
    return rows, s, off


def dense_reward(s0, off0, s1, off1, finished0):
    """The base reward with dense_progress: float32 of ds, wrapped at +-50, zero off the track or for a car that had finished."""
    ds = np.asarray(s1, dtype=np.float64) - np.asarray(s0, dtype=np.float64)
    ds = np.where(ds >= 50.0, ds - 100.0, ds)
    ds = np.where(ds < -50.0, ds + 100.0, ds)
    ds = np.where(np.asarray(off0, dtype=bool) | np.asarray(off1, dtype=bool) | np.asarray(finished0, dtype=bool), 0.0, ds)
    return ds.astype(np.float32)


def penalised(base, off_track, off_track_penalty=0.0, wall=None, wall_penalty=0.0, car=None, car_penalty=0.0):
    """The penalties of ftgp_device_io_signals and ftgp_device_io_contacts on a base reward: binary32 subtractions, in this order."""
    r = np.asarray(base, dtype=np.float32).copy()
    r = np.where(np.asarray(off_track, dtype=bool), r - np.float32(off_track_penalty), r).astype(np.float32)
    if wall is not None:
        r = np.where(np.asarray(wall, dtype=bool), r - np.float32(wall_penalty), r).astype(np.float32)
    if car is not None:
        r = np.where(np.asarray(car, dtype=bool), r - np.float32(car_penalty), r).astype(np.float32)
    return r


def polyline_frame(path, pose):
    """Independent of the header: for every pose and EVERY segment i -> i + 1 of the closed polyline, the distance to the segment
    (np.hypot), the signed offset from it (through the tangent's angle) and the position i + t; and the yaw of every pose.
    Returns (dist [n, 100], lat [n, 100], theta [100], s [n, 100], yaw [n])."""
    path, pose = np.asarray(path, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    p0, p1 = path, np.roll(path, -1, axis=0)
    e = p1 - p0
    ln = np.hypot(e[:, 0], e[:, 1])
    theta = np.arctan2(e[:, 1], e[:, 0])
    ux, uy = np.cos(theta), np.sin(theta)
    r = pose[:, None, 0:2] - p0[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ln > 0.0, np.clip((r[..., 0] * ux + r[..., 1] * uy) / ln, 0.0, 1.0), 0.0)
    foot = p0[None] + t[..., None] * e[None]
    w = pose[:, None, 0:2] - foot
    dist = np.hypot(w[..., 0], w[..., 1])
    lat = ux * w[..., 1] - uy * w[..., 0]
    s = np.arange(PATH_POINTS)[None] + t
    yaw = 2.0 * np.arctan2(pose[:, 6], pose[:, 3])
    return dist, lat, theta, s, yaw


# ---------------------------------------------------------------------------------------------------------------------- paths
def square_path(duplicate=None):
    """A square of side 12.5, counter-clockwise from (0, 0), 25 points per side half a unit apart: every coordinate is dyadic.  Point 0 =
    (0, 0), 25 = (12.5, 0), 50 = (12.5, 12.5), 75 = (0, 12.5), 99 = (0, 0.5).  duplicate = k: point k + 1 is put on point k."""
    i = 0.5 * np.arange(25)
    z, top = np.zeros(25), np.full(25, 12.5)
    p = np.concatenate([np.stack([i, z], 1), np.stack([top, i], 1), np.stack([12.5 - i, top], 1), np.stack([z, 12.5 - i], 1)])
    if duplicate is not None:
        p[duplicate + 1] = p[duplicate]
    return p


SKEW_SHIFT = (8.1, -24.3)
SKEW_POINT_99 = (3.800696369503287, -7.398052024670745)
SKEW_WRAP_POSE = (7.687704582750535, -24.629698178119828)


def skew_path():
    """The square with point 11 on point 10, moved by SKEW_SHIFT (not dyadic) into a 40 x 40 field, and with point 99 moved far
    away to SKEW_POINT_99: Y_99 + 1.0 * (Y_0 - Y_99) then rounds one ulp below Y_0, so that wherever both segments around point 0 clamp
    to it (the outside of that corner) segment A = 99 -> 0 is nearer than B by that ulp: a = 99 with t = 1, which no pose reaches in
    exact arithmetic (the docstring of tests/test_device_frame.py), and s = 100 wraps to 0."""
    p = square_path(duplicate=10) + np.array(SKEW_SHIFT)
    p[99] = SKEW_POINT_99
    return p
