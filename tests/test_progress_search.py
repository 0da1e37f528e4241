"""K3's nearest-point search (`closest = distances.argmin()`, custom.py:1341-1342) pinned in every form the library has, exact ties
included: the oracle's loop, `progress_lane` behind ftgp_set_pose / ftgp_eval_progress and every reset, and both lane layouts of the
in-step search (four lanes per car with two exchanges; sixteen lanes per car with four).

The reference is the numpy model of tests/progress_model.py (binary64, no lanes: argmin's first minimum).  The scenes put cars at rest
on a wall-free map whose centre-line is a ring of lattice points, so that two -- or all hundred -- points are equidistant to the bit:
the strict `d < best` inside a lane's loop and the `lower index wins` of the lane exchanges are then decided at every seam of both
layouts (`ring`) and between lanes, quads and halves of a row far apart (`ring37`); `off_track = best > 1.0` is decided at
dist2 == 1.0 and one ulp to either side.  A car at rest does not move in a step, so set_pose + step(1) runs the in-step search at
exactly the pose that was set (asserted bit for bit).

CPU: the oracle against the model.  GPU: each workgroup shape in a fresh process (tests/progress_child.py) against the model and
against an oracle twin, with the shape asserted from ftgp_create's verbose line; and the four G5 traces with the in-step search in its
four-lane form.
"""
import functools
import os
import re

import numpy as np
import pytest

from ft_grandprix_amd import capi
from ft_grandprix_amd.track import load_track
from tests import children
from tests import progress_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "progress_child.py")


# --------------------------------------------------------------------------------------------------------------- the model's own ground
@pytest.mark.parametrize("order", pm.ORDERS)
def test_ring_poses_are_exact_ties(order):
    pm.check_pool_is_exact(order)
    path = pm.ring_path(order)
    assert sorted(map(tuple, path)) == sorted(map(tuple, pm.ring_path("ring")))
    c, dist2, off, tied = pm.nearest(path, pm.pose_pool())
    assert tied[:201].all() and not tied[201:301].any() and (dist2[201:301] == 0.0).all() and c[0] == 0
    assert off[301:].any() and not off[:301].any()
    kinds = pm.lane_order_kinds(order)
    print(order, kinds)
    if order == "ring":                      # neighbours: the later rank sits lower only across 99 | 0
        assert kinds == {"four": (1, 3), "sixteen": (1, 14)}, kinds
    else:                                    # ... on ring37 on either side, in both layouts
        assert min(kinds["four"]) > 10 and min(kinds["sixteen"]) > 10, kinds


# --------------------------------------------------------------------------------------------------------------- the oracle (CPU)
@pytest.mark.parametrize("via", ["eval", "step"])
@pytest.mark.parametrize("order", pm.ORDERS)
def test_oracle_search_meets_the_model_on_exact_ties(oracle, order, via):
    """set_pose + eval_progress and set_pose + step(1): completion, off_track and centre_dist2 of the whole pool, bit for bit."""
    track, pool = pm.ring_track(order), pm.pose_pool()
    seen = None
    for n, spawn_mode in ((7, 0), (3, 1)):
        with capi.Env(oracle, track, n_envs=n, cars_per_env=1, n_rays=8, lap_target=pm.LAP_TARGET, spawn_mode=spawn_mode) as e:
            model = pm.Model(np.broadcast_to(track.path, (n, 100, 2)), [pm.spawn_offset(spawn_mode, env, 0) for env in range(n)])
            model.update(e.pose()[:, 0:2])                   # the reset ran the search at the spawn pose: on a point, completion 0
            assert (model.completion == 0).all() and (model.dist2 == 0.0).all()
            np.testing.assert_array_equal(e.progress()[:, 1], model.completion)
            np.testing.assert_array_equal(e.centre_dist2(), model.dist2)
            seen = pm.run_pool(e, model, pool, via, seen=seen, what=f"oracle, {order}, {n} envs")
    print(order, via, seen)
    pm.assert_seen(seen)


def test_oracle_search_is_not_contracted_on_arbitrary_doubles(oracle):
    """300 seeded poses around the `track` asset's centre-line: centre_dist2 equals the model's three unfused operations bit for bit,
    and differs from a model with an exactly fused fma(dx, dx, dy * dy) on some pose (47 of the 300 here): a build that contracts the
    sum would be seen."""
    t = load_track("track")
    path = np.asarray(t.path, dtype=np.float64)
    rng = np.random.default_rng(17)
    xy = path[rng.integers(100, size=300)] + rng.uniform(-0.9, 0.9, (300, 2))
    n = 300
    with capi.Env(oracle, t, n_envs=n, cars_per_env=1, n_rays=8, lap_target=pm.LAP_TARGET) as e:
        pose = e.pose()
        pose[:, 0:2], pose[:, 7:] = xy, 0.0
        e.set_pose(pose)
        e.eval_progress()
        got, p = e.centre_dist2(), e.progress()
    c, dist2, off, tied = pm.nearest(path, xy)
    assert not tied.any() and off.any() and not off.all()
    np.testing.assert_array_equal(got, dist2)
    np.testing.assert_array_equal(p[:, 5], off)
    np.testing.assert_array_equal(p[~off, 1], (c[~off] - 10) % 100)
    fused = pm.fused_dist2(path, xy)
    differ = int((fused != dist2).sum())
    print(f"fused products change the minimum's bits on {differ} of {n} poses")
    assert differ > 0 and (fused != got).any()


# --------------------------------------------------------------------------------------------------------------- the GPU part
run_child = functools.partial(children.run_child, CHILD, timeout=120)          # this module's child script and time limit


def workgroup_cars(out):
    """Cars per workgroup of every handle the child created, from ftgp_create's lines."""
    return [int(a) for a in re.findall(r"ftgp_create: (\d+) cars x \d+ waves per workgroup", out)]


# scenario: (envs, FTGP_CARS_PER_BLOCK, spawn_mode, cars per workgroup that must have run)
SHAPES = {
    "one_car_a_workgroup": (3, None, 0, 1),        # sixteen lanes per car, one row of lanes live
    "four_cars": (4, 4, 1, 4),                     # sixteen lanes per car at its limit (4 * 16 = 64)
    "five_cars": (5, 5, 0, 5),                     # the first shape of four lanes per car: 20 live lanes
    "sixteen_cars": (16, 16, 1, 16),               # four lanes per car, all 64 lanes
    "ragged": (19, 8, 1, 8),                       # workgroups of 8, 8 and 3 cars: both forms in one launch
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gpu_in_step_search_meets_the_model_on_exact_ties(shape):
    n, cpb, spawn_mode, cars = SHAPES[shape]
    out = run_child("pool", n_envs=n, cars_per_block=cpb, spawn_mode=spawn_mode, via="step")
    assert workgroup_cars(out) == [cars, cars], out[-2000:]                     # a handle on `ring`, one on `ring37`


@pytest.mark.gpu
def test_gpu_in_step_search_follows_each_track_of_a_multi_track_handle():
    """`ring` and `ring37` in one handle, five envs each, a workgroup of five cars per track: the multi-track instance of the step kernel
    in the four-lane form, every workgroup on its own track's path."""
    out = run_child("two_tracks", n_envs=10, cars_per_block=8, spawn_mode=1)
    assert workgroup_cars(out) == [8], out[-2000:]


@pytest.mark.gpu
def test_gpu_progress_lane_meets_the_model_on_exact_ties():
    """set_pose + eval_progress, and what reset() leaves: completion 0 and dist2 0.0 for every car."""
    out = run_child("pool", n_envs=7, cars_per_block=None, spawn_mode=1, via="eval")
    assert workgroup_cars(out) == [1, 1], out[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("trace", ["forward", "reverse_start", "back_and_forth", "fast_jumps"])
def test_gpu_g5_progress_block_in_the_four_lane_form(trace):
    """The reference's progress block executed verbatim (fixture g5_progress.npz) against the in-step search with four lanes per car:
    8 envs at the fixture's car count in workgroups of 8 cars (6 with three cars per env)."""
    out = run_child("g5", trace=trace)
    cars = workgroup_cars(out)
    assert len(cars) == 2 and cars[0] == cars[1] and cars[0] in (6, 8) and cars[0] >= 5, out[-2000:]
