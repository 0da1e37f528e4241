"""Child process of tests/test_crowded_envs.py: one GPU scenario per process.  Exit status 0 = the scenario held.

    python tests/crowded_child.py <scenario> [json options]

Every scenario runs envs of 6 to 8 cars (a few of 2 and 5 for the binary64 models) on the product, against the CPU oracle bit for bit
and -- `rays`, `contacts` -- against the binary64 models of tests/crowded_model.py.  FTGP_VERBOSE is set: ftgp_create's lines about
the workgroup shape and the inter-vehicle test go to stderr, where the parent reads them.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ["FTGP_VERBOSE"] = "1"

from tests import crowded_model as T  # noqa: E402
from tests.crowded_model import FINISHERS, finish_by_teleport  # noqa: E402
from tests.helpers import libs, open_field, same  # noqa: E402


def pair(product, oracle, track, **kw):
    from ft_grandprix_amd import capi
    g, o = capi.Env(product, track, **kw), capi.Env(oracle, track, **kw)
    oracle.dll.oracle_set_threads(o.h, 8)
    return g, o


def set_rest_pose(e, pos, yaw):
    pose = e.pose()
    pose[:, 0:2] = pos
    pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    pose[:, 7:] = 0.0
    e.set_pose(pose)


def roster_of(cpe):
    return T.ROSTER[cpe]


def drive(envs, policy, n):
    for e in envs:
        e.rollout(policy, n)


# ------------------------------------------------------------------------------------------------------------------ section A
def smallest(opt):
    """One env of 6 cars, 90 rays, one step: the first thing that ever runs a crowded env on the device."""
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("track"), n_envs=1, cars_per_env=6, n_rays=90)
    with g, o:
        g.step(1); o.step(1)
        same(g, o, "one env of 6 cars, one step")
    print("smallest ok")


def rays(opt):
    """A ray scene of section A on the product: the binary64 model's assertions."""
    product, _ = libs()
    T.check_rays(product, tuple(opt["scene"]))
    print("rays ok")


def contacts(opt):
    """A contact scene of section A on the product: the binary64 model's assertions for the step from rest; then product = oracle after
    that step and after 200 more under the random policy."""
    product, oracle = libs()
    if "scene" in opt:
        cpe, R, half_width, n_envs, seed = opt["scene"]
        T.check_pile_up(product, tuple(opt["scene"]))
        pos, yaw = T.thrown(cpe, half_width, n_envs, seed)
    else:
        cpe, R = opt["cars_per_env"], 36
        T.check_touching_pairs(product, cpe)
        pos, yaw = T.touching_pairs(product.default_vehicle(), cpe)
    g, o = pair(product, oracle, open_field(), n_envs=len(pos) // cpe, cars_per_env=cpe, n_rays=R, seed=9)
    with g, o:
        for e in (g, o):
            set_rest_pose(e, pos, yaw)
            e.step(1)
        same(g, o, "one step from rest")
        drive((g, o), "random", 200)
        same(g, o, "200 steps of the random policy after it")
    print("contacts ok")


# ------------------------------------------------------------------------------------------------------------------ section B
def roster(opt):
    """B.1: the reference's roster (or one device policy for every car) on `track`, reference spawn: launches of 1, 1, 60 and 240 steps,
    a reset, 30 more."""
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    cpe, R, policy = opt["cars_per_env"], opt["n_rays"], opt["policy"]
    g, o = pair(product, oracle, load_track("track"), n_envs=opt.get("n_envs", 24), cars_per_env=cpe, n_rays=R, spawn_mode=0, lap_target=3)
    with g, o:
        if policy == "per_car":
            for e in (g, o):
                e.set_car_policies(roster_of(cpe))
        for n in (1, 1, 60, 240):
            drive((g, o), policy, n)
            same(g, o, f"{cpe} cars, {R} rays, {policy}: after a launch of {n} steps")
        g.reset(); o.reset()
        same(g, o, "after the reset")
        drive((g, o), policy, 30)
        same(g, o, f"{cpe} cars, {R} rays, {policy}: 30 steps after the reset")
        print(f"roster ok: kernel {g.kernel_name()}")


def shapes(opt):
    """B.2: one env and two envs per workgroup x 16, 5 and 1 waves, 5 envs (the last two-env workgroup is one env short): equal to each other
    and to the oracle."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    cpe, R = opt["cars_per_env"], opt.get("n_rays", 90)
    t = load_track("track")
    kw = dict(n_envs=5, cars_per_env=cpe, n_rays=R, spawn_mode=0, seed=21, lap_target=2)
    envs = []
    for cpb in (cpe, 2 * cpe):
        for wpb in (16, 5, 1):
            os.environ["FTGP_CARS_PER_BLOCK"], os.environ["FTGP_WAVES_PER_BLOCK"] = str(cpb), str(wpb)
            envs.append(capi.Env(product, t, **kw))
    del os.environ["FTGP_CARS_PER_BLOCK"], os.environ["FTGP_WAVES_PER_BLOCK"]
    o = capi.Env(oracle, t, **kw)
    for e in envs + [o]:
        e.set_car_policies(roster_of(cpe))
    for n in (1, 250):
        drive(envs + [o], "per_car", n)
        for k, e in enumerate(envs):
            for name in ("lidar", "pose", "progress", "ctrl"):
                np.testing.assert_array_equal(getattr(e, name)(), getattr(envs[0], name)(), err_msg=f"shape {k} against shape 0 after {n} steps: {name}")
            same(e, o, f"shape {k} after {n} steps")
    for e in envs + [o]:
        e.close()
    print("shapes ok")


def large(opt):
    """B.2: a batch large enough to get two envs per workgroup by itself: 1100 envs x 7 cars x 36 rays, every env against the oracle."""
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("circle"), n_envs=1100, cars_per_env=7, n_rays=36, spawn_mode=0, seed=8)
    with g, o:
        drive((g, o), "nidc", 60)
        same(g, o, "60 steps")
        g.reset(); o.reset()
        drive((g, o), "nidc", 7)
        same(g, o, "7 steps after the reset")
    print("large ok")


def fakelidar(opt):
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("track"), n_envs=6, cars_per_env=7, n_rays=90, spawn_mode=0, lidar_mode="fakelidar", lap_target=2)
    with g, o:
        for e in (g, o):
            e.set_car_policies(roster_of(7))
        for n in (1, 150):
            drive((g, o), "per_car", n)
            same(g, o, f"FAKELIDAR, 7 cars: after {n} steps")
    print("fakelidar ok")


def bubble_wrap(opt):
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("track"), n_envs=9, cars_per_env=7, n_rays=90, spawn_mode=0, bubble_wrap=True)
    with g, o:
        for n in (1, 300):
            drive((g, o), "random", n)
            same(g, o, f"bubble_wrap, 7 cars: after {n} steps")
    print("bubble wrap ok")


def tricycle(opt):
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("track"), n_envs=8, cars_per_env=6, n_rays=90, spawn_mode=0, seed=4, dt=0.0075, vehicle=product.tricycle_vehicle())
    with g, o:
        for n in (1, 300):
            drive((g, o), "random", n)
            same(g, o, f"tricycle, 6 cars: after {n} steps")
        assert np.abs(g.pose()[:, 7:9]).max() > 0.2
    print("tricycle ok")


def fan(opt):
    """A caller's fan: the group bound does not cover it, every mask is 0xff."""
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    R = 90
    ang = np.deg2rad(360.0 / R * np.arange(R) - 90.0 + 0.37)
    ang[R // 2:] += 3e-5
    dirs = np.stack([np.sin(ang), -np.cos(ang)], axis=1)
    g, o = pair(product, oracle, load_track("track"), n_envs=7, cars_per_env=8, n_rays=R, spawn_mode=0, fan_dirs=dirs)
    with g, o:
        for e in (g, o):
            e.set_car_policies(roster_of(8))
        for n in (1, 40, 200):
            drive((g, o), "per_car", n)
            same(g, o, f"a caller's fan, 8 cars: after {n} steps")
    print("fan ok")


def masked_reset(opt):
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    g, o = pair(product, oracle, load_track("track"), n_envs=10, cars_per_env=8, n_rays=90, spawn_mode=0)
    with g, o:
        for e in (g, o):
            e.set_car_policies(roster_of(8))
        drive((g, o), "per_car", 120)
        same(g, o, "before the masked reset")
        mask = (np.arange(10) % 2 == 1).astype(np.uint8)
        g.reset(mask); o.reset(mask)
        same(g, o, "after the masked reset")
        st = g.steps()
        assert (st[mask == 1] == 0).all() and (st[mask == 0] == 120).all()
        drive((g, o), "per_car", 120)
        same(g, o, "120 steps after the masked reset")
    print("masked reset ok")


def finished_mates(opt):
    """B.3: five of the sixteen cars of two 8-car envs finish (slots 4 to 7 among them): they turn invisible, touch nothing, get the null
    driver and read 0."""
    from ft_grandprix_amd.track import load_track
    product, oracle = libs()
    cpe, t = 8, load_track("track")
    g, o = pair(product, oracle, t, n_envs=3, cars_per_env=cpe, n_rays=1080, spawn_mode=0, lap_target=1)
    with g, o:
        g.step(1); o.step(1)
        before = g.lidar()
        same(g, o, "at the spawn")
        finish_by_teleport((g, o), t, cpe)
        same(g, o, "after the teleports")
        done = np.zeros(3 * cpe, dtype=bool)
        for env, slot in FINISHERS:
            done[env * cpe + slot] = True
        np.testing.assert_array_equal(o.progress()[:, 4] != 0, done, err_msg="who has finished (oracle)")
        np.testing.assert_array_equal(g.progress()[:, 4] != 0, done, err_msg="who has finished")
        g.step(1); o.step(1)
        same(g, o, "one step after the last finish")
        after = g.lidar()
        np.testing.assert_array_equal(after[done], 0.0)
        racing = ~done
        racing[2 * cpe:] = False                                    # env 2 is the control: nobody finished there
        changed = (after[racing] != before[racing]).any(axis=1)
        assert changed.any(), "no racing car sees anything else after its mates have finished"
        drive((g, o), "fast", 200)
        same(g, o, "200 steps of fast after the finishes")
        np.testing.assert_array_equal(g.lidar()[done], 0.0)
        np.testing.assert_array_equal(g.ctrl()[done], 0.0)
        print(f"finished mates ok: {int(changed.sum())} racing cars of envs 0 and 1 see something else")


def randomised(opt):
    """B.4: test_randomised_worlds with 6 to 8 cars per env."""
    from ft_grandprix_amd.track import synthetic_oval
    product, oracle = libs()
    case = opt["case"]
    rng = np.random.default_rng(2000 + case)
    w = int(rng.integers(300, 900)); h = int(rng.integers(260, 700))
    t = synthetic_oval(width=w, height=h, half_width_px=float(rng.uniform(14, 30)), wall_px=float(rng.uniform(0.8, 2.5)),
                       name=f"crowd{case}", frame=("mjcf", "pixel")[case % 2] if case % 3 else "mjcf")
    cars = int(rng.choice([6, 7, 8]))
    n_rays = int(rng.choice([8, 24, 90, 333, 720, 1080]))
    envs = int(rng.integers(3, 40))
    policy = str(rng.choice(["nidc", "fast", "per_car", "per_car", "random", "lobotomy"]))
    v = product.default_vehicle()
    v.friction = float(rng.uniform(0.3, 1.5))
    kw = dict(n_envs=envs, cars_per_env=cars, n_rays=n_rays, spawn_mode=int(rng.integers(0, 2)), seed=int(rng.integers(1, 10 ** 6)),
              lap_target=0 if case == 0 else int(rng.integers(1, 4)), bubble_wrap=bool(rng.integers(0, 2)), vehicle=v)
    names = [str(x) for x in rng.choice(["nidc", "fast", "random", "lobotomy"], cars)]
    g, o = pair(product, oracle, t, **kw)
    with g, o:
        if policy == "per_car":
            for e in (g, o):
                e.set_car_policies(names)
        for n in (1, int(rng.integers(2, 40)), int(rng.integers(40, 260))):
            drive((g, o), policy, n)
            same(g, o, f"case {case}: {cars} cars, {n_rays} rays, {envs} envs, {policy} {names if policy == 'per_car' else ''}, after {n} steps")
    print(f"randomised ok: case {case}: {w} x {h}, {cars} cars, {n_rays} rays, {envs} envs, {policy}")


def puck_margin(opt):
    """B.6: a vehicle whose puck lies only `margin` inside its box behind, mates at the far end of a wall-free map, heading away: the
    specification's min(box, puck) is not the box's time there, and the product must give the oracle's bits."""
    from ft_grandprix_amd import capi
    product, oracle = libs()
    n_envs = opt.get("n_envs", 400)
    v = T.slim_vehicle(product, opt["margin"])
    got = T.far_mates_scan(product, v, n_envs)
    want = T.far_mates_scan(oracle, v, n_envs)
    box = T.far_mates_scan(oracle, v, n_envs, box_only=True)
    differ = got != want
    print(f"margin {opt['margin']}: {int((want >= 0).sum())} hits, the oracle's min(box, puck) differs from its box alone on {int((want != box).sum())} rays "
          f"(by up to {np.abs(want - box).max():.2e}); product != oracle on {int(differ.sum())} rays")
    assert (want != box).any(), "the scene does not show the puck ahead of the box"
    if differ.any():
        k = tuple(np.argwhere(differ)[0])
        raise AssertionError(f"product != oracle on {int(differ.sum())} rays, first (car, ray) {k}: {got[k]!r} against {want[k]!r}")
    print("puck margin ok")


def bundled_vehicles(opt):
    """B.6: both bundled vehicles keep the short path of the inter-vehicle test on every bundled track (the parent reads ftgp_create's line)."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    product, _ = libs()
    for name in ("track", "circle", "small-circle", "inkscape"):
        for v in (product.default_vehicle(), product.tricycle_vehicle()):
            capi.Env(product, load_track(name), n_envs=2, cars_per_env=4, n_rays=90, vehicle=v).close()
    print("bundled vehicles ok")


SCENARIOS = {f.__name__: f for f in (smallest, rays, contacts, roster, shapes, large, fakelidar, bubble_wrap, tricycle, fan, masked_reset,
                                     finished_mates, randomised, puck_margin, bundled_vehicles)}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
