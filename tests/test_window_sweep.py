"""Window-only sweeps: inside a launch whose drivers read the scan, every step but the last marches only the rays the drivers read --
ranges[0] and ranges[n/8 : n - n/8] -- and stores no range (plan_window_table in ftgp_api.hip, lidar_groups / lidar_fake in
ftgp_kernels.hip).  No caller can tell: after any launch every array is what a full sweep on every step gives.  The GPU scenarios run in
tests/window_sweep_child.py; the table itself is checked on the host (tools/plan_check.cpp, tests/test_plan_host.py)."""
import functools
import os
import re

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "window_sweep_child.py")
run_child = functools.partial(children.run_child, CHILD, timeout=300)


def both_kinds_of_handle(out):
    """The scenario made handles with the window-only table (of fewer tasks than the full list, where the fan has a whole unread group) and,
    under FTGP_SCAN_EVERY_STEP, without it."""
    return re.search(r"ftgp_create: \d+ of them on the window-only steps of a launch", out) and "ftgp_create: FTGP_SCAN_EVERY_STEP" in out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rangefinder", "fakelidar"])
@pytest.mark.parametrize("cars", [1, 4])
def test_multi_step_launches_equal_the_oracle_bit_for_bit(cars, mode):
    """lidar (every ray), pose, ctrl, progress, race_steps and snapshot after rollout(p, 7), after rollout(p, 3) + rollout(p, 4) and after
    rollout(p, 7) under FTGP_SCAN_EVERY_STEP=1, each against 7 steps of the oracle: fast and nidc, 24 envs on `track`, 1080 / 90 / 36 rays."""
    out = run_child("oracle", cars=cars, mode=mode)
    assert "oracle ok" in out and both_kinds_of_handle(out)


@pytest.mark.gpu
def test_a_car_that_finishes_inside_a_launch_reads_zero_on_every_ray():
    out = run_child("finished")
    assert "finished ok" in out


@pytest.mark.gpu
def test_roster_of_fast_and_nidc_equals_the_oracle():
    out = run_child("roster")
    assert "roster ok" in out and both_kinds_of_handle(out)


@pytest.mark.gpu
def test_network_driver_launch_equals_the_same_launch_with_every_step_swept():
    out = run_child("network")
    assert "network ok" in out and both_kinds_of_handle(out)
