"""The window-only steps' own cut of the live rays (plan_window_table, ftgp_window_cut.h): 13 full group-marches per car at 1080 rays -- four
pairs over the sideways zone, four single groups over the forward cone, one gather task (kind 3) for what both leave over and ray 0.  No
caller can tell: a ray's range does not depend on the lane or the group that carries it.

Host: tools/plan_check.cpp runs the table check (tools/plan_window_check.h) over fans at each edge of the rule, beside its counted matrix.
GPU: the scenarios of tests/window_recut_child.py against the oracle, bit for bit."""
import functools
import os
import re
import subprocess

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHILD = os.path.join(ROOT, "tests", "window_recut_child.py")
run_child = functools.partial(children.run_child, CHILD, timeout=300)

# window-only tasks per car with the default switches: pairs + single groups + gathers, the cheapest pairs split in two at the tail
# (FTGP_PAIR_TAIL) as far as the first table's task count allows
WINDOW_TASKS = {128: 2, 512: 6, 1080: 11, 1083: 13}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("plan_recut") / "plan_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tools", "plan_check.cpp"), "-o", out, "-ldl", "-w"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FTGP_")}
    return subprocess.run([out], capture_output=True, text=True, env=env)


@pytest.mark.parametrize("cars", [1, 4, 8])
@pytest.mark.parametrize("fan", ["rays 128 cars_per_env {} (no full pair, two gathers)",
                                 "rays 512 cars_per_env {} (zones divide exactly, the gather is ray 0 alone)",
                                 "rays 520 cars_per_env {} (a rest on every zone)",
                                 "rays 520 cars_per_env {} (a caller's fan: singles only)",
                                 "rays 520 cars_per_env {} (FTGP_NO_PAIRS: singles only)",
                                 "rays 640 cars_per_env {} (tail splits give way to the first table's task count)",
                                 "rays 384 cars_per_env {} (FTGP_PAIR_TAIL=0, a list longer than the first table: the first table again)"])
def test_window_table_holds_at_each_edge_of_the_cut_rule(plan_check, fan, cars):
    """Per car slot every live ray drawn exactly once and no other, ray 0 with its flag, window classes, whole pairs and single groups, gather
    entries, ranks and win_group_order, no more tasks than the first table, as few marches as the live rays allow -- and the numbers of
    pairs, single groups and gathers the rule gives for this fan."""
    r = plan_check
    label = "window fan: " + fan.format(cars)
    assert label + ": ok," in r.stdout, r.stdout[-3000:] + r.stderr
    assert "FAIL " + label not in r.stdout, [line for line in r.stdout.splitlines() if line.startswith("FAIL " + label)]


def test_the_counted_matrix_is_what_it_was(plan_check):
    r = plan_check
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert re.search(r"plan_check: 540 configs, \d+ rejected, 0 failures", r.stdout) and "FAIL" not in r.stdout, r.stdout[-2000:]
    # the headline's shape: 11 tasks per car on either list (4 pairs, 4 single groups, 1 gather, 2 pairs split at the tail)
    assert "rays 1080 cars_per_env 1 envs 4096 fan 0 mode 0 no_pairs 0: ok, 8 x 16 waves, 76848 B of LDS, 16 sectors, 11 tasks per car (pairs) (11 window-only)" in r.stdout


def handles(out, rays):
    """The scenario made handles with the window-only list of this fan and, under FTGP_SCAN_EVERY_STEP, without one."""
    return f"ftgp_create: {WINDOW_TASKS[rays]} of them on the window-only steps of a launch" in out and "ftgp_create: FTGP_SCAN_EVERY_STEP" in out


@pytest.mark.gpu
@pytest.mark.parametrize("cars", [1, 4])
@pytest.mark.parametrize("rays", [128, 512, 1080, 1083])
def test_six_steps_equal_the_oracle_bit_for_bit(rays, cars):
    """lidar (every ray), pose, ctrl, progress, race_steps and snapshot after rollout(p, 6), after rollout(p, 2) + rollout(p, 4) and after
    rollout(p, 6) under FTGP_SCAN_EVERY_STEP=1, each against 6 steps of the oracle: fast and nidc, 24 envs on `track`; and one launch of 6 on
    a batch whose last workgroup is short of cars."""
    out = run_child("oracle", rays=rays, cars=cars)
    assert "oracle ok" in out and handles(out, rays), out[-3000:]


@pytest.mark.gpu
def test_fakelidar_mode_decodes_the_gathers():
    out = run_child("fakelidar")
    assert "fakelidar ok" in out and handles(out, 128), out[-3000:]
