"""Child process of tests/test_window_sweep.py: one GPU scenario per process.  Exit status 0 = the scenario held.

    python tests/window_sweep_child.py <scenario> [json options]

Inside a launch whose drivers read the scan, every step but the last sweeps only the rays the drivers read and stores no range
(plan_window_table, lidar_groups).  The criterion throughout: nothing a caller can read after the launch says so -- every array equals,
bit for bit, the oracle's, or what the same launch gives with FTGP_SCAN_EVERY_STEP=1.  ftgp_create reads the switch, so a scenario
sets it in its own environment between two handles; FTGP_VERBOSE makes each ftgp_create say which kind of handle it made, and the test
looks for both lines in the output.
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


def read_back(e):
    return dict(lidar=e.lidar(), pose=e.pose(), ctrl=e.ctrl(), progress=e.progress(), race_steps=e.race_steps(), snapshot=e.snapshot())


def assert_equal_state(a, b, what):
    for k in a:
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        print(f"{what}: {k}: {int((a[k] != b[k]).sum())} of {a[k].size} differ, largest difference {np.nanmax(d) if d.size else 0.0:g}")
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


class every_step:
    """Handles created inside sweep and store every ray on every step."""
    def __enter__(self):
        os.environ["FTGP_SCAN_EVERY_STEP"] = "1"

    def __exit__(self, *exc):
        del os.environ["FTGP_SCAN_EVERY_STEP"]


def launches(lib, track, kw, run):
    """read_back() after run(env) on a fresh handle."""
    with capi.Env(lib, track, **kw) as e:
        run(e)
        return read_back(e)


def oracle(opt):
    """7 steps as one launch, as 3 + 4, and with the switch, against 7 steps of the oracle: 24 envs on `track`, fast and nidc, 1080 / 90 / 36 rays."""
    lib, ora = helpers.libs()
    t = load_track("track")
    cars, mode = int(opt["cars"]), opt["mode"]
    for R in (1080, 90, 36):
        for policy in ("fast", "nidc"):
            kw = dict(n_envs=24, cars_per_env=cars, n_rays=R, spawn_mode=1 if cars == 1 else 0, seed=17, lidar_mode=mode)
            what = f"{mode}, {cars} car(s), {R} rays, {policy}"
            want = launches(ora, t, kw, lambda e: e.rollout(policy, 7))
            assert_equal_state(launches(lib, t, kw, lambda e: e.rollout(policy, 7)), want, f"{what}: one launch of 7")
            assert_equal_state(launches(lib, t, kw, lambda e: (e.rollout(policy, 3), e.rollout(policy, 4))), want, f"{what}: launches of 3 and 4")
            with every_step():
                assert_equal_state(launches(lib, t, kw, lambda e: e.rollout(policy, 7)), want, f"{what}: FTGP_SCAN_EVERY_STEP")
            assert np.abs(want["pose"][:, 7:9]).max() > 0 and (want["lidar"] > 0).any(), f"{what}: nothing happened"
            assert (want["lidar"][:, 1:R // 8] != 0).any(), f"{what}: the rear rays read nothing"
    print("oracle ok")


def finished(opt):
    """A car that finishes inside the launch, before its last step, reads 0 on every ray afterwards (its last sweep is a full one)."""
    lib, ora = helpers.libs()
    t = load_track("circle")
    for R in (1080, 90):
        kw = dict(n_envs=3, n_rays=R, lap_target=1, spawn_mode=1, seed=4)
        with capi.Env(ora, t, **kw) as o:
            n = 0
            while not o.progress()[:, 4].any():          # the step count: from the oracle, six steps past the first finish
                o.rollout("fast", 5); n += 5
                assert n < 40000, "no car finishes a lap"
            o.rollout("fast", 6); n += 6
            want = read_back(o)
        done = want["progress"][:, 4] != 0
        assert done.any(), done
        assert (want["race_steps"][done, 1] < n - 1).all() and (want["race_steps"][done, 1] >= 0).all(), (want["race_steps"], n)
        got = launches(lib, t, kw, lambda e: e.rollout("fast", n))
        assert_equal_state(got, want, f"{R} rays, one launch of {n}")
        np.testing.assert_array_equal(got["lidar"][done], 0.0)
        assert (got["lidar"][~done][:, 1:R // 8] != 0).any(axis=1).all(), "a racing car's rear rays"
        print(f"finished: {R} rays, {n} steps, cars {np.flatnonzero(done)} finished at {want['race_steps'][done, 1]}")
    print("finished ok")


def roster(opt):
    """FTGP_POLICY_PER_CAR mixing fast and nidc against the oracle."""
    lib, ora = helpers.libs()
    t = load_track("track")
    names = ["fast", "nidc", "nidc", "fast"]
    for R in (1080, 90):
        kw = dict(n_envs=24, cars_per_env=4, n_rays=R, spawn_mode=0, seed=23)

        def run(e):
            e.set_car_policies(names)
            e.rollout("per_car", 7)
        want = launches(ora, t, kw, run)
        assert_equal_state(launches(lib, t, kw, run), want, f"roster, {R} rays")
        with every_step():
            assert_equal_state(launches(lib, t, kw, run), want, f"roster, {R} rays: FTGP_SCAN_EVERY_STEP")
    print("roster ok")


def network(opt):
    """A network driver, 5 steps in one launch: the arrays of the same launch with the switch set."""
    from tests import net_model as nm
    lib = capi.load()
    t = load_track("small-circle")
    # 17 inputs = 12 pooled beams + the state; the beams lie inside the drivers' window: rays 8 .. 55 of 64, rays 180 .. 899 of 1080
    for R, cars, pool, first in ((64, 2, 4, 2), (1080, 1, 60, 3)):
        net = nm.random_net(np.random.default_rng(21), (17, 16, 2), pool=pool, max_range=3.0, beam_first=first, use_state=True, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
        kw = dict(n_envs=19, cars_per_env=cars, n_rays=R, spawn_mode=1, seed=5)

        def run(e):
            e.set_net(0, net["layers"], **{k: v for k, v in net.items() if k != "layers"})
            e.rollout("net0", 5)
        with every_step():
            want = launches(lib, t, kw, run)
        assert_equal_state(launches(lib, t, kw, run), want, f"network, {R} rays")
        assert np.abs(want["pose"][:, 7:9]).max() > 0.01, "the cars did not move"
    print("network ok")


SCENARIOS = {"oracle": oracle, "finished": finished, "roster": roster, "network": network}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
