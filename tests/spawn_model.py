"""numpy / Python model of the spawn rule, written from the text of include/ftgp.h (FtgpSpawnRule): the start table of a track, the
list of start points a rule leaves, and the draw of an env's start poses.  Python floats are binary64 and every operation below is
one Python operation, so each rounds once, as the header has it; hashes are Python integers cut to 64 bits.

Shared by tests/test_spawn_rule.py (against the host harness tools/spawn_check.cpp) and tests/spawn_rule_child.py (against the GPU).
"""
import dataclasses
import math

import numpy as np

PATH_POINTS = 100
M64 = (1 << 64) - 1
LEFT, RIGHT = 0, 1


@dataclasses.dataclass
class Rule:
    first_point: int = 0
    n_points: int = PATH_POINTS
    shuffle_grid: bool = False
    margin: float = 0.0
    lateral_frac: float = 0.0
    yaw_tan: float = 0.0

    def kwargs(self):
        """Arguments of capi.Env.set_spawn_rule."""
        return dataclasses.asdict(self)


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u01(h):
    return float(h >> 11) * (1.0 / 9007199254740992.0)


def mul32(h, n):
    return ((h >> 32) * n) >> 32


def spawn_table(track):
    """float64 [100, 4]: x, y, qw, qz -- a car on path point p looks at point p + 1 (math.atan2 / cos / sin: the host's libm)."""
    path = np.asarray(track.path, dtype=np.float64)
    out = np.zeros((PATH_POINTS, 4))
    for p in range(PATH_POINTS):
        q = (p + 1) % PATH_POINTS
        ang = math.atan2(float(path[q, 1]) - float(path[p, 1]), float(path[q, 0]) - float(path[p, 0]))
        out[p] = path[p, 0], path[p, 1], math.cos(ang / 2), math.sin(ang / 2)
    return out


def blocked(track, wall, px, py):
    u = (px - track.origin_x) * (1.0 / track.px_size_x)
    w = (track.origin_y - py) * (1.0 / track.px_size_y)
    ix, iy = math.floor(u), math.floor(w)
    if not (0 <= ix < track.width and 0 <= iy < track.height):
        return True
    return bool(wall[iy, ix])


def clearances(track, table):
    """float64 [100, 2]: clear[p][LEFT / RIGHT] of the header's "Start table" for the spawn entries in `table` ([100, >= 4])."""
    wall = track.wall_mask()
    delta = 0.5 * min(track.px_size_x, track.px_size_y)
    K = int(math.ceil(1.0 / delta))
    clear = np.zeros((PATH_POINTS, 2))
    for p in range(PATH_POINTS):
        X, Y, qw, qz = (float(v) for v in table[p, :4])
        ch, sh = 1.0 - 2.0 * (qz * qz), 2.0 * (qw * qz)
        for side, (nx, ny) in ((LEFT, (-sh, ch)), (RIGHT, (sh, -ch))):
            m = K + 1
            for k in range(K + 1):
                d = float(k) * delta
                if blocked(track, wall, X + d * nx, Y + d * ny):
                    m = k
                    break
            clear[p, side] = delta * float(max(m - 1, 0))
    return clear


def start_table(track, poses=None):
    """float64 [100, 6]: x, y, qw, qz, clear_left, clear_right.  poses: another [100, >= 4] table to take the first four columns from."""
    t = spawn_table(track) if poses is None else np.array(poses, dtype=np.float64)[:, :4]
    return np.concatenate([t, clearances(track, t)], axis=1)


def start_list(table, rule):
    """The window's points, in order, whose clearance is at least the margin on both sides."""
    out = []
    for i in range(rule.n_points):
        p = (rule.first_point + i) % PATH_POINTS
        if table[p, 4] < rule.margin or table[p, 5] < rule.margin:
            continue
        out.append(p)
    return out


def draw_env(seed, G, k, c, rule, table, path, start):
    """The c cars of global env G in episode k.  Returns a dict of arrays over the cars: p, slot, offset (int32), pose = x, y, qw, qz
    (float64 [c, 4]), side (0 left, 1 right) and room (what step 5 had to work with)."""
    hE = splitmix64(splitmix64((seed ^ ((0x5350574E52554C45 + G) & M64)) & M64) ^ (k & M64))
    b = start[mul32(hE, len(start))]
    slot = list(range(c))
    if rule.shuffle_grid:
        h = hE
        for i in range(c - 1, 0, -1):
            h = splitmix64(h)
            j = mul32(h, i + 1)
            slot[i], slot[j] = slot[j], slot[i]
    path = np.asarray(path, dtype=np.float64)
    out = dict(p=np.zeros(c, np.int32), slot=np.array(slot, np.int32), offset=np.zeros(c, np.int32), pose=np.zeros((c, 4)),
               side=np.zeros(c, np.int32), room=np.zeros(c))
    for a in range(c):
        p = (b + 2 * slot[a]) % PATH_POINTS
        hC = splitmix64(hE ^ ((0xD6E8FEB86659FD93 * (a + 1)) & M64))
        w = 2.0 * u01(hC) - 1.0
        v = 2.0 * u01(splitmix64(hC)) - 1.0
        X, Y, qw, qz = (float(t) for t in table[p, :4])
        ch, sh = 1.0 - 2.0 * (qz * qz), 2.0 * (qw * qz)
        side = LEFT if w >= 0 else RIGHT
        room = max(float(table[p, 4 + side]) - rule.margin, 0.0)
        lat = (rule.lateral_frac * w) * room
        x, y = X + lat * (-sh), Y + lat * ch
        t = rule.yaw_tan * v
        nw, nz, m = qw, qz, 1.0                                   # t == 0: the table's quaternion as it is
        if t != 0.0:
            n = math.sqrt(1.0 + t * t)
            cj, sj = 1.0 / n, t / n
            nw, nz = qw * cj - qz * sj, qz * cj + qw * sj
            m = math.sqrt(nw * nw + nz * nz)
        dx, dy = path[:, 0] - x, path[:, 1] - y
        out["p"][a], out["offset"][a] = p, int(np.argmin(dx * dx + dy * dy))       # argmin: the first index of the smallest
        out["pose"][a] = x, y, nw / m, nz / m
        out["side"][a], out["room"][a] = side, room
    return out


def draw_batch(seed, env_base, n_envs, c, episodes, rule, table, path, start):
    """draw_env over envs [env_base, env_base + n_envs), env e in episode episodes[e] (a number = the same for all): arrays
    [n_envs, c(, 4)] under the keys of draw_env."""
    ks = np.broadcast_to(np.asarray(episodes, dtype=np.int64), (n_envs,))
    rows = [draw_env(seed, env_base + e, int(ks[e]), c, rule, table, path, start) for e in range(n_envs)]
    return {key: np.stack([r[key] for r in rows]) for key in rows[0]}
