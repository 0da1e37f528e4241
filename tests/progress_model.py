"""A numpy model of K3's nearest-point search (custom.py:1341-1345) in binary64, the exact centre-lines its ties are decided on, and the
scene that runs a pose pool through a library (the oracle on the CPU: tests/test_progress_search.py; libftgp.so with an oracle twin on
the GPU: tests/progress_child.py).

    d = (path[:, 0] - x) ** 2 + (path[:, 1] - y) ** 2;  c = d.argmin();  dist2 = d[c];  off = dist2 > 1.0
    while not off: completion = (c - offset) % 100; off the track every race field keeps its value

The model has no lanes and no loop over points: argmin takes the first minimum, which is what every form of the search must return.

The exact paths.  x^2 + y^2 = 1105^2 has 108 lattice points (1105 = 5 * 13 * 17).  The first 100 by atan2(y, x), scaled by 2**-11 around
(20, -20), make a ring of radius 0.5396 whose coordinates have 11 fraction bits.  A pose centre + t * ((p_i - centre) + (p_j - centre)) / 2
with t in {1/2, 2} has 13, and every difference, square and sum of the model then is exact: points i and j are equidistant to the bit.
`ring` numbers the points by angular rank (ties between neighbouring indices: every seam of both lane layouts, and 99 | 0); `ring37` puts
rank k at index 37 k % 100 (ties between indices far apart: other lanes, other quads, other halves of a row of sixteen).
"""
import dataclasses
from fractions import Fraction

import numpy as np

CENTRE = np.array([20.0, -20.0])
RADIUS, SCALE = 1105, 2.0 ** -11
LAP_TARGET = 1000                        # no car ever finishes
ORDERS = ("ring", "ring37")


def lattice_points():
    """int64 [100, 2]: the first 100 of the circle's 108 lattice points by atan2(y, x)."""
    r = np.arange(-RADIUS, RADIUS + 1)
    x, y = np.meshgrid(r, r, indexing="ij")
    on = x * x + y * y == RADIUS * RADIUS
    pts = np.stack([x[on], y[on]], axis=1)
    assert len(pts) == 108
    pts = pts[np.argsort(np.arctan2(pts[:, 1], pts[:, 0]), kind="stable")]
    return pts[:100]


def ring_path(order):
    """float64 [100, 2]: the ring in the order `ring` (index = angular rank) or `ring37` (rank k at index 37 k % 100)."""
    by_rank = CENTRE + SCALE * lattice_points()
    if order == "ring":
        return by_rank
    assert order == "ring37"
    path = np.empty_like(by_rank)
    path[37 * np.arange(100) % 100] = by_rank
    return path


def ring_track(order):
    from tests.helpers import open_field
    return dataclasses.replace(open_field(200), path=ring_path(order), name=order)


def spawn_offset(spawn_mode, env, car):
    """The car's progress offset = its spawn index (custom.py:1112; spawn_mode 1: the library's spread over the lap)."""
    return (car + 5) * 2 if spawn_mode == 0 else (10 + 7 * env + 2 * car) % 98


def distances(paths, xy):
    """float64 [n, 100]: paths [n, 100, 2] (or [100, 2] for all), xy [n, 2].  Three array operations, none fused."""
    paths, xy = np.asarray(paths, dtype=np.float64), np.asarray(xy, dtype=np.float64)
    if paths.ndim == 2:
        paths = np.broadcast_to(paths, (len(xy),) + paths.shape)
    return (paths[:, :, 0] - xy[:, None, 0]) ** 2 + (paths[:, :, 1] - xy[:, None, 1]) ** 2


def nearest(paths, xy):
    """(c int [n], dist2 float64 [n], off bool [n], tied bool [n]): the first minimum, its distance, off the track, more than one minimum."""
    d = distances(paths, xy)
    c = d.argmin(axis=1)
    dist2 = d[np.arange(len(d)), c]
    return c, dist2, dist2 > 1.0, (d == dist2[:, None]).sum(axis=1) > 1


def fused_dist2(path, xy):
    """min over the points of fma(dx, dx, dy * dy), the sum a contracting compiler makes of dx * dx + dy * dy: dy * dy rounded, then the
    exact dx * dx + that rounded once (float(Fraction) rounds correctly)."""
    out = np.empty(len(xy))
    for k, (x, y) in enumerate(np.asarray(xy, dtype=np.float64)):
        dx, dy = path[:, 0] - x, path[:, 1] - y
        yy = dy * dy
        out[k] = min(float(Fraction(float(a)) * Fraction(float(a)) + Fraction(float(b))) for a, b in zip(dx, yy))
    return out


class Model:
    """The race fields the search decides, per car: completion (kept while off the track), off_track, dist2."""

    def __init__(self, paths, offsets):
        self.paths = np.asarray(paths, dtype=np.float64)                  # [n, 100, 2]: each car's centre-line
        self.offsets = np.asarray(offsets, dtype=np.int64)
        n = len(self.offsets)
        self.completion, self.off, self.dist2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n)
        self.c, self.tied = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)

    def update(self, xy):
        self.c, self.dist2, self.off, self.tied = nearest(self.paths, xy)
        self.completion = np.where(self.off, self.completion, (self.c - self.offsets) % 100)


# ---------------------------------------------------------------------------------------------------------------------- the poses
def bisector(path_by_rank, k, t):
    """The pose at t times the mid-point of the ring's angular neighbours k and k + 1, seen from the centre."""
    i, j = k % 100, (k + 1) % 100
    return CENTRE + t * ((path_by_rank[i] - CENTRE) + (path_by_rank[j] - CENTRE)) / 2


def boundary_poses():
    """On the ring point (20 + 1105 * 2**-11, -20) plus (1, 0): dist2 == 1.0, not off the track; x one ulp higher: off; one ulp lower."""
    x, y = 20.0 + RADIUS * SCALE + 1.0, -20.0
    return [(x, y), (np.nextafter(x, np.inf), y), (np.nextafter(x, -np.inf), y)]


def pose_pool(seed=5):
    """float64 [401, 2], the same poses for both orders: the centre (a 100-way tie); the 100 two-way ties at t = 1/2 and the 100 at
    t = 2; the 100 poses on a point; the three boundary poses; 97 seeded poses with |x - cx|, |y - cy| < 1.5 (its corners are off the
    track)."""
    ring = ring_path("ring")
    pool = [tuple(CENTRE)]
    pool += [tuple(bisector(ring, k, t)) for t in (0.5, 2.0) for k in range(100)]
    pool += [tuple(p) for p in ring]
    pool += boundary_poses()
    rng = np.random.default_rng(seed)
    pool += [tuple(CENTRE + rng.uniform(-1.5, 1.5, 2)) for _ in range(97)]
    return np.array(pool)


def lanes4(i):
    return i // 25


def lanes16(i):
    return i // 7


def lane_order_kinds(order):
    """Of the 100 tied neighbour pairs (rank k, rank k + 1): how many have the later rank's point in a lower lane than the earlier
    one's, how many in a higher lane -- {layout: (lower, higher)} for the four-lane and the sixteen-lane layout."""
    k = np.arange(100)
    a, b = (k, (k + 1) % 100) if order == "ring" else (37 * k % 100, 37 * (k + 1) % 100)
    return {name: (int((lane(b) < lane(a)).sum()), int((lane(b) > lane(a)).sum())) for name, lane in (("four", lanes4), ("sixteen", lanes16))}


def check_pool_is_exact(order):
    """What the scenes rest on, from the model alone: the centre is a 100-way tie; every bisector pose at t in {1/4, 1/2, 1, 2} is an
    exact two-way tie of its two points, which are the only minima, on the track; the boundary poses are == 1, > 1, < 1."""
    path, ring = ring_path(order), ring_path("ring")
    rank_at = np.arange(100) if order == "ring" else 37 * np.arange(100) % 100       # index of angular rank k
    d = distances(path, CENTRE[None])[0]
    assert (d == d[0]).all() and d[0] == 0.29111504554748535, d
    for t in (0.25, 0.5, 1.0, 2.0):
        xy = np.array([bisector(ring, k, t) for k in range(100)])
        d = distances(path, xy)
        i, j = rank_at, rank_at[(np.arange(100) + 1) % 100]
        rows = np.arange(100)
        assert (d[rows, i] == d[rows, j]).all() and (d[rows, i] == d.min(axis=1)).all() and (d[rows, i] <= 1.0).all(), t
        assert ((d == d.min(axis=1)[:, None]).sum(axis=1) == 2).all(), t
    c, dist2, off, _ = nearest(path, np.array(boundary_poses()))
    assert dist2[0] == 1.0 and not off[0] and dist2[1] > 1.0 and off[1] and dist2[2] < 1.0 and not off[2], dist2
    assert (c == c[0]).all()


# ---------------------------------------------------------------------------------------------------------------------- the scene
COUNTS = ("poses", "tied", "off", "boundary", "c0", "c99")


def run_pool(env, model, pool, via, twins=(), passes=2, seen=None, what="", blocks=None):
    """The pool through `env` (cars_per_env = 1: car = env) and the model, round after round.

    pool: float64 [L, 2].  blocks: [(first car, cars)], the runs of cars that walk the pool on their own (default: the whole batch;
    the env blocks of a multi-track handle).  Round r puts pool pose (r m + k) % L on slot (k + r) % m of a block of m cars, so a pose
    meets another slot on every pass; every pose runs in every block.  via "step": set_pose + step(1), the in-step search (a car at
    rest on the wall-free map does not move: pose() afterwards must be what was set, bit for bit); "eval": set_pose + eval_progress,
    the one-lane search.
    twins: [(oracle env, first car, cars)]: the same calls on an oracle handle per block of cars; progress(), lap_times() and
    race_steps() must be equal arrays.  Returns the counts (COUNTS) of what the model saw."""
    n, L = env.n_cars, len(pool)
    assert env.cars_per_env == 1 and pool.shape == (L, 2) and via in ("step", "eval")
    seen = seen if seen is not None else dict.fromkeys(COUNTS, 0)
    base = env.pose()
    base[:, 3], base[:, 4:7], base[:, 7:] = 1.0, 0.0, 0.0                       # heading 0: set_pose's normalisation changes no bit
    visited = np.zeros((n, L), dtype=bool)
    blocks = blocks or [(0, n)]
    assert sum(m for _, m in blocks) == n
    rounds = -(-passes * L // min(m for _, m in blocks))
    prev = env.progress()
    for r in range(rounds):
        slot = np.concatenate([first + (np.arange(m) + r) % m for first, m in blocks])
        take = np.concatenate([(r * m + np.arange(m)) % L for _, m in blocks])
        pose = base.copy()
        pose[slot, 0:2] = pool[take]
        for e, first, cars in [(env, 0, n)] + list(twins):
            e.set_pose(pose[first:first + cars])
            e.step(1) if via == "step" else e.eval_progress()
        at = f"{what}: round {r} ({via})"
        np.testing.assert_array_equal(env.pose(), pose, err_msg=f"{at}: a car moved")
        model.update(pose[:, 0:2])
        p, d2 = env.progress(), env.centre_dist2()
        hint = f"\nmodel c {model.c.tolist()}\ntied {model.tied.astype(int).tolist()}"
        np.testing.assert_array_equal(d2, model.dist2, err_msg=f"{at}: centre_dist2{hint}")
        np.testing.assert_array_equal(p[:, 5], model.off, err_msg=f"{at}: off_track{hint}")
        np.testing.assert_array_equal(p[:, 1], model.completion, err_msg=f"{at}: completion{hint}")
        keep = np.delete(np.arange(p.shape[1]), 5)
        np.testing.assert_array_equal(p[model.off][:, keep], prev[model.off][:, keep], err_msg=f"{at}: off the track a race field changed")
        prev = p
        cnt, ring = env.lap_times()
        steps = env.race_steps()
        for o, first, cars in twins:
            s = slice(first, first + cars)
            np.testing.assert_array_equal(p[s], o.progress(), err_msg=f"{at}: progress() against the oracle{hint}")
            oc, oring = o.lap_times()
            np.testing.assert_array_equal(cnt[s], oc, err_msg=f"{at}: lap counts")
            np.testing.assert_array_equal(ring[s], oring, err_msg=f"{at}: lap times")
            np.testing.assert_array_equal(steps[s], o.race_steps(), err_msg=f"{at}: race_steps()")
        visited[slot, take] = True
        seen["poses"] += n; seen["tied"] += int(model.tied.sum()); seen["off"] += int(model.off.sum())
        seen["boundary"] += int((model.dist2 == 1.0).sum()); seen["c0"] += int((model.c == 0).sum()); seen["c99"] += int((model.c == 99).sum())
    for first, cars in blocks:
        ran = visited[first:first + cars].any(axis=0)
        assert ran.all(), f"{what}: {int((~ran).sum())} pool poses never ran on cars {first} .. {first + cars - 1}"
    return seen


def assert_seen(seen):
    for k in COUNTS:
        assert seen[k] > 0, (k, seen)
