"""Envs of 6, 7 and 8 cars (ftgp_create admits 8; the reference ships a seven-car roster, template/cars/all.json), and the two
inter-vehicle operations -- rays against env-mates, car-car contact forces -- against binary64 models that owe nothing to the oracle
or the kernel.

A. The models (numpy, tests/crowded_model.py).  On a map without walls every range is -1 or a hit on an env-mate, so the scan isolates the
   inter-vehicle ray test; from rest (no velocities, no controls, no walls) one step gives (vx, vy, wz) = dt (Fx / m, Fy / m, Tz / Izz)
   of the car-car contact forces alone.  The same assertions hold for the oracle (CPU tests) and the product (GPU tests):
     rays      |range - model| <= 1e-4 wherever both agree about hit / miss; they may disagree only on rays that the MODEL calls
               grazing (its own answer flips when the observer's yaw turns by +-1e-6 rad), and grazing rays are at most 1e-3 of the
               rays that hit or graze.  Measured against the model (oracle and product alike, the scenes below, 3.4 million rays): worst
               error 6.9e-5 (8 cars spread over 20 units, a hit at 7.3; 2.3e-5 for the scenes of half-width 1.5 and less), grazing
               share 0 to 3.4e-4 per scene (7 grazing rays in all), no hit / miss flip.
     contacts  max |(vx, vy, wz) - model| <= 1e-12 max |model| per scene (binary64 on both sides, another order of summation;
               measured 3e-14 to 3.5e-13, oracle and product alike).
     witnesses every mate slot >= 4 is the nearest hit of at least 10 rays in each ray scene of 6+ cars; every ordered (slot, mate)
               pair touches in the constructed contact scenes; at least a quarter of the cars of a pile-up feel a force.
B. Crowded envs on the GPU against the oracle, bit for bit: the reference's roster, workgroups of one and two envs, modes and events,
   finished mates, randomised worlds, and the slim margin between the LiDAR puck and the chassis box.

Every GPU scenario runs in a fresh child process (tests/crowded_child.py) under a time limit, the smallest first.  If a child ends by a
signal, an abort or its time limit, every later child of the session is refused (tests/children.py).
"""
import functools
import os

import numpy as np
import pytest

from tests import children
from tests.crowded_model import (PILE_UPS, RAY_SCENES, check_pile_up, check_rays, check_touching_pairs, far_mates_scan, puck_margin_needed,
                                 scene_id, slim_vehicle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "crowded_child.py")


# ------------------------------------------------------------------------------------------------------------- A on the CPU
@pytest.mark.parametrize("scene", RAY_SCENES, ids=scene_id)
def test_oracle_rays_against_env_mates_meet_the_binary64_model(oracle, scene):
    check_rays(oracle, scene)


@pytest.mark.parametrize("scene", PILE_UPS, ids=scene_id)
def test_oracle_contact_forces_of_a_pile_up_meet_the_binary64_model(oracle, scene):
    check_pile_up(oracle, scene)


@pytest.mark.parametrize("cpe", [2, 5, 6, 7, 8])
def test_oracle_contact_forces_of_every_slot_pair_meet_the_binary64_model(oracle, cpe):
    check_touching_pairs(oracle, cpe)


# ------------------------------------------------------------------------------------------------------------- B.6 on the CPU
def test_oracle_box_alone_is_min_of_box_and_puck_at_the_derived_margin(oracle):
    """The bound behind VehLds::puck_in_box: with the puck `puck_margin_needed` inside the box, the specification's min(box, puck) is the
    box's time to the bit for mates at the far end of the map -- and with a slim margin it is not (the scene can tell)."""
    r0 = oracle.default_vehicle().lidar_ring_radius
    need = puck_margin_needed(np.hypot(40.0, 40.0), r0)
    assert 0.0158 < need < 0.0160
    for v in (oracle.default_vehicle(), oracle.tricycle_vehicle()):       # the bundled vehicles keep the short path on a 40 x 40 map
        r = v.lidar_ring_radius
        have = min(v.lidar_x - r - v.box_xmin, v.box_xmax - v.lidar_x - r, v.lidar_y - r - v.box_ymin, v.box_ymax - v.lidar_y - r)
        assert have >= puck_margin_needed(np.hypot(40.0, 40.0), r), have
    for margin, same in ((need, True), (0.0015, False), (0.005, False)):
        v = slim_vehicle(oracle, margin)
        both, box = far_mates_scan(oracle, v, 600), far_mates_scan(oracle, v, 600, box_only=True)
        differ = both != box
        print(f"margin {margin:.4f}: {int((both >= 0).sum())} hits, min(box, puck) != box on {int(differ.sum())} rays, "
              f"largest difference {np.abs(both - box).max():.2e}")
        assert (both >= 0).sum() > 10000
        assert differ.any() != same, margin


# ------------------------------------------------------------------------------------------------------------- the GPU part
run_child = functools.partial(children.run_child, CHILD, timeout=300)          # this module's child script and time limit


def workgroup_shapes(out):
    """(cars, waves) per workgroup of every handle the child created, from ftgp_create's lines."""
    import re
    return [(int(a), int(b)) for a, b in re.findall(r"ftgp_create: (\d+) cars x (\d+) waves per workgroup", out)]


def inter_vehicle_paths(out):
    import re
    return re.findall(r"ftgp_create: inter-vehicle rays test (the box only|the box and the puck's circle)", out)


@pytest.mark.gpu
def test_gpu_smallest_crowded_env_first():
    out = run_child("smallest")
    assert workgroup_shapes(out) == [(6, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", RAY_SCENES, ids=scene_id)
def test_gpu_rays_against_env_mates_meet_the_binary64_model(scene):
    run_child("rays", scene=scene)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", PILE_UPS, ids=scene_id)
def test_gpu_contact_forces_of_a_pile_up_meet_the_binary64_model(scene):
    run_child("contacts", scene=scene)


@pytest.mark.gpu
@pytest.mark.parametrize("cpe", [2, 5, 6, 7, 8])
def test_gpu_contact_forces_of_every_slot_pair_meet_the_binary64_model(cpe):
    run_child("contacts", cars_per_env=cpe)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["per_car", "fast", "random"])
@pytest.mark.parametrize("n_rays", [90, 1080])
@pytest.mark.parametrize("cpe", [6, 7, 8])
def test_gpu_reference_roster_matches_the_oracle(cpe, n_rays, policy):
    """template/cars/all.json's drivers (the first six, all seven, those and one more `fast`), reference spawn; small batches run ONE env
    per workgroup: workgroups of 6, 7 and 8 cars."""
    out = run_child("roster", cars_per_env=cpe, n_rays=n_rays, policy=policy)
    assert workgroup_shapes(out) == [(cpe, 16)]
    assert ("<true, false, true>" if policy == "per_car" else "<true, false, false>") in out         # multi-car; the roster instance for per_car only


@pytest.mark.gpu
@pytest.mark.parametrize("cpe", [6, 7, 8])
def test_gpu_one_and_two_crowded_envs_per_workgroup_give_the_same_bits(cpe):
    out = run_child("shapes", cars_per_env=cpe)
    assert workgroup_shapes(out) == [(cpb, wpb) for cpb in (cpe, 2 * cpe) for wpb in (16, 5, 1)]


@pytest.mark.gpu
def test_gpu_large_batch_takes_two_seven_car_envs_per_workgroup():
    out = run_child("large")
    assert workgroup_shapes(out) == [(14, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ["fakelidar", "bubble_wrap", "tricycle", "fan", "masked_reset"])
def test_gpu_crowded_modes_and_events(scenario):
    run_child(scenario)


@pytest.mark.gpu
def test_gpu_finished_mates_in_slots_four_to_seven():
    run_child("finished_mates")


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(8))
def test_randomised_crowded_worlds(case):
    run_child("randomised", case=case)


@pytest.mark.gpu
@pytest.mark.parametrize("margin", [0.0015, 0.005])
def test_gpu_slim_puck_margin_takes_the_circle_test(margin):
    """Before the margin was derived from the error bound (1e-3 was asked for), these vehicles took the box alone and were up to 7e-3 off
    the specification at the far end of the map."""
    out = run_child("puck_margin", margin=margin)
    assert inter_vehicle_paths(out) == ["the box and the puck's circle"]


@pytest.mark.gpu
def test_gpu_bundled_vehicles_keep_the_short_inter_vehicle_test():
    out = run_child("bundled_vehicles")
    assert inter_vehicle_paths(out) == ["the box only"] * 8
