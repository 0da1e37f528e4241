"""The window-only sweep's plain draws (ftgp_device.h, FTGP_TASK_MASKED; lidar_groups<MULTI, true>): a pair or a single group of the window-only
table holds 64 live rays a group, all of them in the drivers' window and none of them ray 0, so the sweep runs it with every lane live -- no
lane mask, one LDS store for the delivery -- and leaves the draw of a car slot the workgroup does not have by a scalar branch.  No caller can
tell: everything equals the oracle's, bit for bit.

Host: tools/plan_check.cpp (tools/plan_window_check.h) asserts that a plain draw is of kind 0 or 1 -- the table holds no kind 2 --, covers 64
live rays a group, lies inside the window and holds no ray 0, that every gather is marked, and that a table which is the first table again is
marked entry for entry (run by tests/test_plan_host.py and tests/test_window_recut.py, which build the program: not built a third time here).
GPU: the scenarios of tests/window_shell_child.py -- 13 envs in workgroups of 8 cars, the last one short of cars."""
import functools
import os
import subprocess
import sys

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "window_shell_child.py")
run_child = functools.partial(children.run_child, CHILD, timeout=300)

# window-only tasks per car with the default switches (pairs, single groups, gathers; the cheapest pairs split at the tail)
WINDOW_TASKS = {128: 2, 520: 7, 1080: 11, 1083: 13}


def test_the_oracle_alone_makes_both_kinds_of_parked_range():
    """The edge scenario cannot pass vacuously: in the oracle's own batch one car of the first workgroup is finished (every range 0) and
    another has rays that start off the image (range -1), beside six racing cars."""
    r = subprocess.run([sys.executable, CHILD, "edge_oracle_alone"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "edge oracle ok" in r.stdout, (r.stdout + r.stderr)[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("rays,cars", [(1080, 1), (520, 1), (128, 1), (1083, 1), (1080, 4)])
def test_six_steps_equal_the_oracle_bit_for_bit(rays, cars):
    """lidar, pose, ctrl, progress and race_steps after rollout(p, 6), after rollout(p, 2) + rollout(p, 4) and after rollout(p, 6) under
    FTGP_SCAN_EVERY_STEP=1, each against 6 steps of the oracle: fast and nidc, 13 envs on `track` in workgroups of 8 cars.  1080 rays: pairs,
    single groups and a gather; 520: a rest on every zone; 128: no full pair, two gathers; 1083: single groups only; 4 cars per env: the
    ranks and mate masks of the instantiation with env-mates."""
    out = run_child("oracle", rays=rays, cars=cars)
    assert "oracle ok" in out, out[-3000:]
    assert f"ftgp_create: {WINDOW_TASKS[rays]} of them on the window-only steps of a launch" in out and "ftgp_create: FTGP_SCAN_EVERY_STEP" in out, out[-3000:]


@pytest.mark.gpu
def test_a_finished_car_and_a_car_at_the_image_edge_beside_plain_draws():
    """all_safe is false in the first workgroup -- one car finished, one with its LiDAR centre one pixel from the image's left edge --
    while its other six cars' pairs and single groups run with every lane live."""
    out = run_child("edge")
    assert "edge ok" in out, out[-3000:]
