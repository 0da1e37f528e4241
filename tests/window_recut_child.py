"""Child process of tests/test_window_recut.py: one GPU scenario per process.  Exit status 0 = the scenario held.

    python tests/window_recut_child.py <scenario> [json options]

The window-only steps of a launch draw from a list of their own cut (plan_window_table, ftgp_window_cut.h): pairs of 64 + 64 rays over the
sideways zone, single groups over the forward cone, and what is left of both, with ray 0, in gather tasks whose lanes take their rays from
runs (gather_lanes in ftgp_kernels.hip).  A ray's range depends on its car's frame and its own index, not on the lane or the group that
carries it: every array a caller can read equals, bit for bit, the oracle's.  The controls after 6 steps pin every window sample the
drivers read on the five window-only steps.  ftgp_create reads the FTGP_* switches, so a scenario sets them in its own environment between
two handles.
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
for name in ("FTGP_SCAN_EVERY_STEP", "FTGP_CARS_PER_BLOCK"):
    os.environ.pop(name, None)

STEPS = 6


def read_back(e):
    return dict(lidar=e.lidar(), pose=e.pose(), ctrl=e.ctrl(), progress=e.progress(), race_steps=e.race_steps(), snapshot=e.snapshot())


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


def compare(lib, ora, t, kw, policy, what, ragged=None):
    want = launches(ora, t, kw, lambda e: e.rollout(policy, STEPS))
    assert_equal_state(launches(lib, t, kw, lambda e: e.rollout(policy, STEPS)), want, f"{what}: one launch of {STEPS}")
    assert_equal_state(launches(lib, t, kw, lambda e: (e.rollout(policy, 2), e.rollout(policy, 4))), want, f"{what}: launches of 2 and 4")
    with switch("SCAN_EVERY_STEP", 1):
        assert_equal_state(launches(lib, t, kw, lambda e: e.rollout(policy, STEPS)), want, f"{what}: FTGP_SCAN_EVERY_STEP")
    R = kw["n_rays"]
    assert np.abs(want["pose"][:, 7:9]).max() > 0 and (want["lidar"] > 0).any(), f"{what}: nothing happened"
    assert (want["lidar"][:, 1:R // 8] != 0).any(), f"{what}: the rear rays read nothing"
    if ragged:              # the same cars in workgroups of `cars_per_block`, the last one short of cars: it draws tasks of cars it does not have
        cars_per_block, n_envs = ragged
        kw = dict(kw, n_envs=n_envs)
        assert (n_envs * kw["cars_per_env"]) % cars_per_block, "not a ragged batch"
        want = launches(ora, t, kw, lambda e: e.rollout(policy, STEPS))
        with switch("CARS_PER_BLOCK", cars_per_block):
            assert_equal_state(launches(lib, t, kw, lambda e: e.rollout(policy, STEPS)), want, f"{what}: {n_envs} envs in workgroups of {cars_per_block} cars")


def oracle(opt):
    """6 steps as one launch, as 2 + 4, and with FTGP_SCAN_EVERY_STEP, against 6 steps of the oracle: 24 envs on `track`, fast and nidc; then a
    batch whose last workgroup is short of cars."""
    lib, ora = helpers.libs()
    t = load_track("track")
    R, cars = int(opt["rays"]), int(opt["cars"])
    for policy in ("fast", "nidc"):
        kw = dict(n_envs=24, cars_per_env=cars, n_rays=R, spawn_mode=1 if cars == 1 else 0, seed=17)
        compare(lib, ora, t, kw, policy, f"{cars} car(s), {R} rays, {policy}", ragged=(5, 24) if cars == 1 else (8, 23))
    print("oracle ok")


def fakelidar(opt):
    """FAKELIDAR mode decodes the same table (lidar_fake): 128 rays, two gathers and no other window-only task."""
    lib, ora = helpers.libs()
    t = load_track("track")
    for cars in (1, 4):
        kw = dict(n_envs=24, cars_per_env=cars, n_rays=128, spawn_mode=1 if cars == 1 else 0, seed=17, lidar_mode="fakelidar")
        compare(lib, ora, t, kw, "fast", f"fakelidar, {cars} car(s), 128 rays, fast")
    print("fakelidar ok")


SCENARIOS = {"oracle": oracle, "fakelidar": fakelidar}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
