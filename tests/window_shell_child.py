"""Child process of tests/test_window_shell.py: one scenario per process.  Exit status 0 = the scenario held.

    python tests/window_shell_child.py <scenario> [json options]

A pair or a single group of the window-only table is a PLAIN draw (ftgp_device.h, FTGP_TASK_MASKED clear): 64 live rays a group, all of them in
the drivers' window, no ray 0.  lidar_groups runs such a draw without a lane mask -- set-up, march, delivery with every lane live -- and skips
the draw of a car slot the workgroup does not have by one scalar branch.  Nothing a caller can read may say so: lidar, pose, ctrl, progress
and race_steps equal the oracle's bit for bit.  Every batch has 13 envs in workgroups of 8 cars, so the last workgroup is short of cars.
ftgp_create reads the FTGP_* switches, so a scenario sets them in its own environment between two handles.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402
from tests import helpers  # noqa: E402

os.environ["FTGP_VERBOSE"] = "1"
os.environ.pop("FTGP_SCAN_EVERY_STEP", None)
os.environ["FTGP_CARS_PER_BLOCK"] = "8"

STEPS, ENVS = 6, 13
FINISHED, AT_EDGE = 2, 5          # cars of the first workgroup (edge scenario)


def read_back(e):
    return dict(lidar=e.lidar(), pose=e.pose(), ctrl=e.ctrl(), progress=e.progress(), race_steps=e.race_steps())


def assert_equal_state(a, b, what):
    for k in a:
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        print(f"{what}: {k}: {int((a[k] != b[k]).sum())} of {a[k].size} differ, largest difference {np.nanmax(d) if d.size else 0.0:g}")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


class switch:
    """Handles created inside see FTGP_<name>=<value>."""
    def __init__(self, name, value):
        self.name, self.value = "FTGP_" + name, str(value)

    def __enter__(self):
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        del os.environ[self.name]


def launches(lib, track, kw, run):
    """read_back() after run(env) on a fresh handle."""
    with capi.Env(lib, track, **kw) as e:
        run(e)
        return read_back(e)


def plain(policy):
    return lambda e: e.rollout(policy, STEPS), lambda e: (e.rollout(policy, 2), e.rollout(policy, 4))


def edge(policy, t, veh):
    """Before the launches: car FINISHED is carried round the centre line until it has its one lap (lap_target = 1: four one-step launches, the
    line crossed forwards on the last), car AT_EDGE is put down with its LiDAR centre one pixel inside the image's left edge (less than the ring radius: some of its rays start off the image)."""
    def prepare(e):
        pose = e.pose()
        c0 = int(np.argmin(((t.path - pose[FINISHED, :2]) ** 2).sum(axis=1)))
        for ahead in (45, 90, 96, 2):
            pose = e.pose()
            pose[FINISHED, :2] = t.path[(c0 + ahead) % len(t.path)]
            pose[FINISHED, 7:] = 0.0
            e.set_pose(pose)
            e.rollout(policy, 1)
        pose = e.pose()
        pose[AT_EDGE, :] = 0.0
        pose[AT_EDGE, 0] = t.origin_x + 1.0 * t.px_size_x - veh.lidar_x
        pose[AT_EDGE, 1] = t.origin_y - 0.5 * t.height * t.px_size_y
        pose[AT_EDGE, 3] = 1.0
        e.set_pose(pose)
    return lambda e: (prepare(e), e.rollout(policy, STEPS)), lambda e: (prepare(e), e.rollout(policy, 2), e.rollout(policy, 4))


def compare(lib, ora, t, kw, runs, what, want=None):
    """6 steps as one launch, as 2 + 4 and under FTGP_SCAN_EVERY_STEP against the oracle's 6 steps (`want`: already computed)."""
    one, split = runs
    want = want if want is not None else launches(ora, t, kw, one)
    assert_equal_state(launches(lib, t, kw, one), want, f"{what}: one launch of {STEPS}")
    assert_equal_state(launches(lib, t, kw, split), want, f"{what}: launches of 2 and 4")
    with switch("SCAN_EVERY_STEP", 1):
        assert_equal_state(launches(lib, t, kw, one), want, f"{what}: FTGP_SCAN_EVERY_STEP")
    return want


def oracle(opt):
    """13 envs on `track`, fast and nidc: the window-only list of this fan against the oracle."""
    lib, ora = helpers.libs()
    t = load_track("track")
    R, cars = int(opt["rays"]), int(opt["cars"])
    for policy in ("fast", "nidc"):
        kw = dict(n_envs=ENVS, cars_per_env=cars, n_rays=R, spawn_mode=1 if cars == 1 else 0, seed=17)
        want = compare(lib, ora, t, kw, plain(policy), f"{cars} car(s), {R} rays, {policy}")
        assert np.abs(want["pose"][:, 7:9]).max() > 0 and (want["lidar"] > 0).any(), "nothing happened"
        assert (ENVS * cars) % 8, "not a ragged batch"
    print("oracle ok")


def edge_oracle_alone(opt):
    """CPU: the oracle's own batch of the edge scenario holds both kinds of range the fix-up path makes -- -1 on a ray that starts off the image, 0 on
    every ray of the finished car -- beside racing cars in the same workgroup of 8."""
    ora = helpers.load_oracle()
    t = load_track("track")
    kw = dict(n_envs=ENVS, n_rays=1080, lap_target=1, spawn_mode=1, seed=17)
    for policy in ("fast", "nidc"):
        want = launches(ora, t, kw, edge(policy, t, ora.default_vehicle())[0])
        check_edge_batch(want, policy)
    print("edge oracle ok")


def check_edge_batch(want, policy):
    done = want["progress"][:, 4] != 0
    assert list(np.flatnonzero(done)) == [FINISHED], f"{policy}: finished cars {np.flatnonzero(done)}"
    assert (want["lidar"][FINISHED] == 0.0).all(), f"{policy}: the finished car reads something"
    off = want["lidar"][AT_EDGE] == -1.0
    assert off.any() and not off.all(), f"{policy}: {int(off.sum())} rays of the car at the edge start off the image"
    racing = [c for c in range(8) if c not in (FINISHED, AT_EDGE)]
    assert (want["lidar"][racing] > 0).any(axis=1).all() and not (want["lidar"][racing] == -1.0).any(), f"{policy}: the racing cars of the first workgroup"
    print(f"{policy}: car {FINISHED} finished at step {want['race_steps'][FINISHED, 1]}, {int(off.sum())} rays of car {AT_EDGE} start off the image")


def edge_gpu(opt):
    """The same batch on the device: all_safe is false in a workgroup that also runs plain draws."""
    lib, ora = helpers.libs()
    t = load_track("track")
    kw = dict(n_envs=ENVS, n_rays=1080, lap_target=1, spawn_mode=1, seed=17)
    for policy in ("fast", "nidc"):
        runs = edge(policy, t, ora.default_vehicle())
        want = launches(ora, t, kw, runs[0])
        check_edge_batch(want, policy)
        compare(lib, ora, t, kw, runs, f"edge, {policy}", want=want)
    print("edge ok")


SCENARIOS = {"oracle": oracle, "edge_oracle_alone": edge_oracle_alone, "edge": edge_gpu}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
