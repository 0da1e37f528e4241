"""Binary64 models of the two inter-vehicle operations -- rays against env-mates, car-car contact forces -- that owe nothing to the
oracle or the kernel, their scenes and their checkers; the oracle runs them on the CPU (tests/test_crowded_envs.py), the product in
tests/crowded_child.py, and the wall models (tests/walls_model.py) and the device-step tests borrow scenes from here.

On a map without walls every range is -1 or a hit on an env-mate, so the scan isolates the inter-vehicle ray test; from rest (no
velocities, no controls, no walls) one step gives (vx, vy, wz) = dt (Fx / m, Fy / m, Tz / Izz) of the car-car contact forces alone.
The assertions and what was measured: the docstring of tests/test_crowded_envs.py.
"""
import numpy as np

from ft_grandprix_amd import capi
from tests.helpers import open_field

TOL = 1e-4                 # the project's tolerance for floating-point outputs (BASELINE north star)
GRAZE_EPS = 1e-6           # rad: a ray whose hit / miss answer in the MODEL changes under this turn of the observer is grazing
GRAZE_CAP = 1e-3           # share of grazing rays among the rays that hit or graze
CONTACT_RTOL = 1e-12
DT = 0.004
CENTRE = np.array([20.0, -20.0])          # of open_field()

# template/cars/all.json: the reference's seven-car roster (drivers by name), and one more `fast` for the eighth slot
ROSTER7 = ["nidc", "fast", "nidc", "nidc", "nidc", "nidc", "nidc"]
ROSTER = {6: ROSTER7[:6], 7: ROSTER7, 8: ROSTER7 + ["fast"]}


# ------------------------------------------------------------------------------------------------------------- A: the models
def ray_model(v, pos, yaw, R, cpe, turn=0.0):
    """Ranges [n, R] (-1 = nothing hit) and the mate slot that gave each, in binary64.  Car i: LiDAR centre c = p + R(psi) (lidar_x,
    lidar_y); ray j looks along d = R(psi + turn) (sin phi_j, -cos phi_j), phi_j = radians(360 j / R - 90) (mushr.em.xml:112-117), and
    starts at c - r0 d.  Against every env-mate, in the mate's frame: slab test on the chassis box and circle test on the puck, an origin
    inside either reads 0; the minimum over the mates."""
    n, r0 = len(pos), v.lidar_ring_radius
    out, who = np.full((n, R), -1.0), np.full((n, R), -1)
    phi = np.deg2rad(360.0 / R * np.arange(R) - 90.0)
    bx, by = np.sin(phi), -np.cos(phi)
    for i in range(n):
        c, s = np.cos(yaw[i] + turn), np.sin(yaw[i] + turn)
        c0, s0 = np.cos(yaw[i]), np.sin(yaw[i])
        dx, dy = c * bx - s * by, s * bx + c * by
        ox = pos[i, 0] + c0 * v.lidar_x - s0 * v.lidar_y - r0 * dx
        oy = pos[i, 1] + s0 * v.lidar_x + c0 * v.lidar_y - r0 * dy
        best, slot = np.full(R, np.inf), np.full(R, -1)
        first = i - i % cpe
        for k in range(cpe):
            m = first + k
            if m == i:
                continue
            cb, sb = np.cos(yaw[m]), np.sin(yaw[m])
            rx, ry = ox - pos[m, 0], oy - pos[m, 1]
            lx, ly = cb * rx + sb * ry, -sb * rx + cb * ry
            ldx, ldy = cb * dx + sb * dy, -sb * dx + cb * dy
            with np.errstate(divide="ignore", invalid="ignore"):
                t1, t2 = (v.box_xmin - lx) / ldx, (v.box_xmax - lx) / ldx
                t3, t4 = (v.box_ymin - ly) / ldy, (v.box_ymax - ly) / ldy
            tmin, tmax = np.maximum(np.minimum(t1, t2), np.minimum(t3, t4)), np.minimum(np.maximum(t1, t2), np.maximum(t3, t4))
            tb = np.where(tmax >= np.maximum(tmin, 0.0), np.maximum(tmin, 0.0), np.inf)
            px, py = lx - v.lidar_x, ly - v.lidar_y
            bq, cq = px * ldx + py * ldy, px * px + py * py - r0 * r0
            disc = bq * bq - cq
            with np.errstate(invalid="ignore"):
                tc = -bq - np.sqrt(disc)
            tc = np.where(disc >= 0, np.where(tc < 0, np.where(cq < 0, 0.0, np.inf), tc), np.inf)
            t = np.minimum(tb, tc)
            nearer = t < best
            best, slot = np.where(nearer, t, best), np.where(nearer, k, slot)
        out[i], who[i] = np.where(np.isfinite(best), best, -1.0), slot
    return out, who


def contact_model(v, pos, yaw, cpe, dt=DT):
    """(dvx, dvy, dwz) [n, 3] of one step from rest, and how many circle pairs touch per (slot, mate slot).  Every ordered pair of
    env-mates, every pair of their contact circles (contact_x[i] on each car's axis, radius contact_radius): for 0 < d < 2 radius the force
    stiffness (2 radius - d) e / d on the first car (e = centre difference), torque r x f about its origin."""
    n, cx, r2 = len(pos), np.array(list(v.contact_x)), 2.0 * v.contact_radius
    F, touching = np.zeros((n, 3)), np.zeros((cpe, cpe), dtype=int)
    for i in range(n):
        first = i - i % cpe
        for k in range(cpe):
            m = first + k
            if m == i:
                continue
            for a in cx:
                for b in cx:
                    ra = np.array([np.cos(yaw[i]) * a, np.sin(yaw[i]) * a])
                    rb = np.array([np.cos(yaw[m]) * b, np.sin(yaw[m]) * b])
                    e = pos[i] + ra - pos[m] - rb
                    d = np.hypot(e[0], e[1])
                    if 0.0 < d < r2:
                        f = v.contact_stiffness * (r2 - d) * e / d
                        F[i, 0] += f[0]; F[i, 1] += f[1]; F[i, 2] += ra[0] * f[1] - ra[1] * f[0]
                        touching[i % cpe, k] += 1
    return np.stack([dt * F[:, 0] / v.mass, dt * F[:, 1] / v.mass, dt * F[:, 2] / v.izz], axis=1), touching


# ------------------------------------------------------------------------------------------------------------- A: the scenes
# (cars per env, rays, half-width of the square the cars are thrown into, envs, seed): the seeds are fixed, so the grazing share of every
# scene is a constant of the test
RAY_SCENES = [(cpe, 1080, s, 24, 100 + 10 * cpe + k) for cpe in (2, 5, 6, 7, 8) for k, s in enumerate((0.6, 1.5, 10.0))] + \
             [(6, 90, 0.8, 24, 301), (8, 90, 1.5, 24, 302), (7, 360, 1.5, 24, 303)]
# pile-ups: 0.6 for the crowded envs; two and five cars need a smaller square to stand as densely (a quarter of the cars must touch)
PILE_UPS = [(2, 36, 0.2, 40, 502), (5, 36, 0.4, 40, 505), (6, 36, 0.6, 40, 406), (7, 36, 0.6, 40, 507), (8, 36, 0.6, 40, 408)]
PAIR_YAWS = (0.0, 0.7, 2.4, -1.9)         # of the second car relative to the first, in the constructed contact scenes


def scene_id(s):
    return f"{s[0]}cars-{s[1]}rays-s{s[2]}"


def thrown(cpe, half_width, n_envs, seed):
    """Positions uniform in a square about the map's centre, yaws uniform: cars may overlap."""
    rng = np.random.default_rng(seed)
    n = n_envs * cpe
    yaw = rng.uniform(-np.pi, np.pi, n)
    return CENTRE + rng.uniform(-half_width, half_width, (n, 2)), yaw


def touching_pairs(v, cpe):
    """For every ordered pair (a, b) of slots and every relative yaw one env: cars a and b 0.9 * 2 * contact_radius apart, every other
    car metres away (on a circle of radius 8 about the pair)."""
    rng = np.random.default_rng(77 + cpe)
    pos, yaw = [], []
    for a in range(cpe):
        for b in range(cpe):
            if a == b:
                continue
            for rel in PAIR_YAWS:
                p, y = np.zeros((cpe, 2)), rng.uniform(-np.pi, np.pi, cpe)
                at = CENTRE + rng.uniform(-3.0, 3.0, 2)
                bearing = rng.uniform(-np.pi, np.pi)
                for k in range(cpe):
                    p[k] = at + 8.0 * np.array([np.cos(2 * np.pi * k / cpe), np.sin(2 * np.pi * k / cpe)])
                p[a] = at
                p[b] = at + 0.9 * 2.0 * v.contact_radius * np.array([np.cos(bearing), np.sin(bearing)])
                y[b] = y[a] + rel
                pos.append(p); yaw.append(y)
    return np.concatenate(pos), np.concatenate(yaw)


def one_step_from_rest(lib, cpe, R, pos, yaw):
    """(scan, pose after the step): the scan of step(1) belongs to the pose the step starts from."""
    n = len(pos)
    with capi.Env(lib, open_field(), n_envs=n // cpe, cars_per_env=cpe, n_rays=R) as e:
        if lib.has("set_threads"):
            lib.fn("set_threads")(e.h, 8)
        pose = e.pose()
        pose[:, 0:2] = pos
        pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        pose[:, 7:] = 0.0
        e.set_pose(pose)
        e.step(1)
        return e.lidar().astype(np.float64), e.pose()


def ray_scene_model(v, scene):
    """The model's side of a ray scene -- positions, yaws, ranges, nearest mate, grazing rays -- with its witnesses and the grazing cap."""
    cpe, R, half_width, n_envs, seed = scene
    pos, yaw = thrown(cpe, half_width, n_envs, seed)
    want, who = ray_model(v, pos, yaw, R, cpe)
    plus, _ = ray_model(v, pos, yaw, R, cpe, GRAZE_EPS)
    minus, _ = ray_model(v, pos, yaw, R, cpe, -GRAZE_EPS)
    grazing = ((want < 0) != (plus < 0)) | ((want < 0) != (minus < 0))
    near = (want >= 0) | grazing
    share = grazing.sum() / near.sum()
    nearest = [int((who == k).sum()) for k in range(cpe)]
    print(f"{scene_id(scene)}: {want.size} rays, {int((want >= 0).sum())} hits, grazing {int(grazing.sum())} ({share:.2e} of the rays that hit or graze), "
          f"nearest hits per mate slot {nearest}, longest range {want.max():.2f}")
    assert share <= GRAZE_CAP, (scene, share)
    assert (want >= 0).sum() >= 100, f"{scene_id(scene)}: only {int((want >= 0).sum())} rays hit"
    for k in range(4, cpe):
        assert nearest[k] >= 10, f"{scene_id(scene)}: mate slot {k} is the nearest hit of {nearest[k]} rays only"
    return pos, yaw, want, grazing


def check_rays(lib, scene):
    v = lib.default_vehicle()
    pos, yaw, want, grazing = ray_scene_model(v, scene)
    got, _ = one_step_from_rest(lib, scene[0], scene[1], pos, yaw)
    flip = (got < 0) != (want < 0)
    err = np.where(flip | (want < 0), 0.0, np.abs(got - want))
    worst = np.unravel_index(np.argmax(err), err.shape)
    print(f"{scene_id(scene)}: worst |range - model| {err.max():.3e} (car {worst[0]}, ray {worst[1]}: {got[worst]!r} against {want[worst]!r}), "
          f"hit / miss flips {int(flip.sum())}, outside the grazing rays {int((flip & ~grazing).sum())}")
    bad = np.argwhere(flip & ~grazing)
    assert len(bad) == 0, f"{scene_id(scene)}: hit / miss differs from the model on rays that do not graze, first (car, ray) {tuple(bad[0])}: " \
                          f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}"
    assert err.max() <= TOL, f"{scene_id(scene)}: car {worst[0]} (slot {worst[0] % scene[0]}) ray {worst[1]}: {got[worst]!r} against {want[worst]!r}"


def check_contacts(lib, cpe, R, pos, yaw, what, pile_up):
    v = lib.default_vehicle()
    want, touching = contact_model(v, pos, yaw, cpe)
    off = touching[~np.eye(cpe, dtype=bool)]
    felt = int((np.abs(want).sum(axis=1) > 0).sum())
    if pile_up:
        assert 4 * felt >= len(pos), f"{what}: only {felt} of {len(pos)} cars feel a force"
    else:
        assert off.min() >= len(PAIR_YAWS), f"{what}: (slot, mate) pairs that never touch\n{touching}"
    _, after = one_step_from_rest(lib, cpe, R, pos, yaw)
    got = after[:, [7, 8, 12]]
    scale = np.abs(want).max()
    dev = np.abs(got - want)
    worst = np.unravel_index(np.argmax(dev), dev.shape)
    print(f"{what}: {felt} of {len(pos)} cars feel a force, fewest touching circle pairs over (slot, mate) {off.min()}, "
          f"max |(vx, vy, wz) - model| / max |model| = {dev.max() / scale:.2e}")
    assert dev.max() <= CONTACT_RTOL * scale, \
        f"{what}: car {worst[0]} (env {worst[0] // cpe}, slot {worst[0] % cpe}) component {worst[1]}: {got[worst]!r} against {want[worst]!r}"


def check_pile_up(lib, scene):
    cpe, R, half_width, n_envs, seed = scene
    pos, yaw = thrown(cpe, half_width, n_envs, seed)
    check_contacts(lib, cpe, R, pos, yaw, f"pile-up of {cpe} cars", True)


def check_touching_pairs(lib, cpe):
    pos, yaw = touching_pairs(lib.default_vehicle(), cpe)
    check_contacts(lib, cpe, 36, pos, yaw, f"touching pairs of {cpe} cars", False)


# ------------------------------------------------------------------------------------------------------------- the puck's margin
def puck_margin_needed(diag, r0):
    """What plan_vehicle asks for before the sweep may leave the puck's circle out: the circle's discriminant is off by up to 5 * 2^-24 D^2
    at D units (largest seen here: 3.9), which moves the puck's near side by that over 2 r0."""
    return 5.0 * 2.0 ** -24 * diag * diag / (2.0 * r0)


def slim_vehicle(lib, margin):
    """The bundled vehicle with its box cut back behind: the puck's rear is `margin` inside the box."""
    v = lib.default_vehicle()
    v.box_xmin = v.lidar_x - v.lidar_ring_radius - margin
    return v


def far_mates(n_envs, seed=3, cpe=4):
    """Car 0 of every env near one corner of the 40 x 40 map, its mates near the opposite one (40 to 55 units away: the diagonal is
    56.6), heading away: the rear, where the puck is, faces the observer."""
    rng = np.random.default_rng(seed)
    pos, yaw = np.zeros((n_envs * cpe, 2)), np.zeros(n_envs * cpe)
    for env in range(n_envs):
        o = np.array([rng.uniform(0.5, 4), -rng.uniform(0.5, 4)])
        pos[env * cpe], yaw[env * cpe] = o, rng.uniform(-np.pi, np.pi)
        for k in range(1, cpe):
            m = np.array([rng.uniform(30, 39.5), -rng.uniform(30, 39.5)])
            pos[env * cpe + k] = m
            yaw[env * cpe + k] = np.arctan2(m[1] - o[1], m[0] - o[0]) + rng.uniform(-0.5, 0.5)
    return pos, yaw


def far_mates_scan(lib, v, n_envs, box_only=False, cpe=4):
    pos, yaw = far_mates(n_envs, cpe=cpe)
    with capi.Env(lib, open_field(), n_envs=n_envs, cars_per_env=cpe, n_rays=1080, vehicle=v) as e:
        if lib.has("set_threads"):
            lib.fn("set_threads")(e.h, 8)
        if box_only:
            lib.fn("set_box_only")(e.h, 1)
        pose = e.pose()
        pose[:, 0:2] = pos
        pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        pose[:, 7:] = 0.0
        e.set_pose(pose)
        e.step(1)
        return e.lidar()


# ------------------------------------------------------------------------------------------------------------- finished mates
FINISHERS = ((0, 1), (0, 4), (0, 6), (1, 5), (1, 7))             # (env, slot)


def finish_by_teleport(envs, track, cpe):
    """Ten steps with the FINISHERS put onto path points start + 25, 50, 75, 99, 0, 1, ... (K3's crossing logic: laps_by_teleport of
    tests/helpers.py); every other car is left alone."""
    path = np.asarray(track.path, dtype=np.float64)
    for ahead in (25, 50, 75, 99, 0, 1, 2, 3, 4, 5):
        for e in envs:
            pose = e.pose()
            for env, slot in FINISHERS:
                q = ((slot + 5) * 2 + ahead) % 100                 # spawn_mode 0: slot s starts on path[(s + 5) * 2] (custom.py:1112)
                a = np.arctan2(path[(q + 1) % 100, 1] - path[q, 1], path[(q + 1) % 100, 0] - path[q, 0])
                row = pose[env * cpe + slot]
                row[0], row[1], row[3], row[6] = path[q, 0], path[q, 1], np.cos(a / 2), np.sin(a / 2)
                row[7:] = 0.0
            e.set_pose(pose)
            e.step(1)
