"""Contact signals of the device step (include/ftgp.h: FTGP_CONTACT_FLOATS, ftgp_device_io_contacts / ftgp_step_device_contacts /
ftgp_contacts_device / ftgp_get_contacts; ft_grandprix_amd/vec.py: DeviceVecEnv(contacts=, terminate_on_wall_contact=,
terminate_on_car_contact=, wall_contact_penalty=, car_contact_penalty=)).

CPU: the binding, the argument checks, the numpy model of the header's text (tests/contacts_model.py) on hand-written poses, and that
model against the two independent binary64 models the project has -- `wall_contact_model` of tests/walls_model.py and
`contact_model` of tests/crowded_model.py -- on their own scenes.

   Counts must agree car by car.  Penetrations before the binary32 rounding agree with r - hypot(...) of those models within
   CONTACT_RTOL (1e-12) of max(the model's penetration, the circle radius): relative to the penetration where it is deep, to the radius
   it is subtracted from where it is shallow (the independent models go through cos / sin of the yaw and np.hypot, the header through
   the quaternion and sqrt).  A car sits on a comparison boundary if the two sides can legitimately
   disagree about a count: a circle within BOUNDARY of touching a pixel or a mate's circle (d2 against r*r), or a centre within
   BOUNDARY pixels of a pixel boundary (division against multiplication by the inverse pixel size decides its window).  Such cars are
   named and left out, at most TIED_CAP (1e-2) of a scene.  Measured: no car on a boundary in any scene (smallest margin 5.1e-6); worst
   deviation 4.4e-16 for walls and 2.3e-15 for cars (20 units from the origin) against bounds of 6.0e-14 to 1.3e-13.

GPU: every scenario runs in a fresh child process (tests/device_contacts_child.py) that imports torch before libftgp.so is loaded, one
at a time, each under a time limit.  A child that ends by a signal, an abort or its time limit fails its test, and every later child
of the session is refused (tests/children.py).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from ft_grandprix_amd import capi
from tests import children
from tests import contacts_model as cm
from tests import crowded_model as TC
from tests import walls_model as TW
from tests.helpers import open_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "device_contacts_child.py")

CONTACT_RTOL = TW.CONTACT_RTOL
TIED_CAP = TW.TIED_CAP
BOUNDARY = 1e-9

WALL_SCENES = ["thrown-97x64", "thrown-fine", "thrown-bubble-wrap", "thrown-tricycle", "leaning", "finished"]
CPU_PILE_UPS = [s for s in TC.PILE_UPS if s[0] in (2, 5, 8)]
GPU_PILE_UPS = [s for s in TC.PILE_UPS if s[0] in (2, 5, 6, 8)]


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_contact_entries():
    assert C.sizeof(capi.FtgpDeviceContacts) == 16
    assert [getattr(capi.FtgpDeviceContacts, f).offset for f in ("terminate_on_wall", "terminate_on_car", "wall_penalty", "car_penalty")] == [0, 4, 8, 12]
    assert C.sizeof(capi.FtgpDeviceStepContacts) == 16 and capi.FtgpDeviceStepContacts.final_contact.offset == 8
    assert capi.CONTACT_FLOATS == cm.CONTACT_FLOATS == len(capi.CONTACT_FIELDS) == 4
    assert capi.CONTACT_FIELDS == ("wall_pen", "car_pen", "wall_count", "car_count")
    lib = capi.load()
    for name in ("device_io_contacts", "step_device_contacts", "contacts_device", "get_contacts"):
        assert name in capi.API_SYMBOLS and lib.has(name), name
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "#define FTGP_CONTACT_FLOATS 4" in header and "#define FTGP_ABI_VERSION 5" in header


@pytest.mark.parametrize("kwargs", [dict(wall_contact_penalty=-0.5), dict(wall_contact_penalty=float("nan")),
                                    dict(wall_contact_penalty=float("inf")), dict(car_contact_penalty=-1.0),
                                    dict(car_contact_penalty=float("nan")), dict(car_contact_penalty=float("inf")),
                                    dict(contacts=True, scan_pool=7)])
def test_device_vec_env_checks_the_contact_arguments_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, **kwargs)


def hand_vehicle():
    """Circles of radius 0.5 at -1, 0 and +1 on the axis; softeners of radius 0.25 at (+-1, +-1)."""
    v = capi.FtgpVehicle()
    v.contact_x[0], v.contact_x[1], v.contact_x[2] = 1.0, 0.0, -1.0
    v.contact_radius = 0.5
    for k, (wx, wy) in enumerate(((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))):
        v.wheel_x[k], v.wheel_y[k] = wx, wy
    v.softener_radius = 0.25
    return v


def hand_track(wall_pixels, w=40, h=40):
    """Pixels of 0.25 x 0.25, the image covers [0, 10] x [-10, 0]: pixel (cx, cy) is [0.25 cx, 0.25 cx + 0.25] x [-0.25 cy - 0.25, -0.25 cy]."""
    wall = np.zeros((h, w), dtype=bool)
    for cx, cy in wall_pixels:
        wall[cy, cx] = True
    return TW.synthetic(wall, 0.25, 0.25, 0.0, 0.0, "hand")


def poses(rows):
    """(x, y, yaw) per car -> rows of ftgp_get_pose."""
    p = np.zeros((len(rows), 13))
    for k, (x, y, yaw) in enumerate(rows):
        p[k, 0], p[k, 1], p[k, 3], p[k, 6] = x, y, math.cos(yaw / 2), math.sin(yaw / 2)
    return p


def test_model_on_hand_written_poses():
    """Every number below is a dyadic rational and the headings are exact (yaw 0: qw = 1, qz = 0), so the expected rows are exact."""
    v, f, none = hand_vehicle(), np.float32, [0]
    row = lambda *a: np.array([a], dtype=f)
    # one wall pixel (20, 20) = [5, 5.25] x [-5.25, -5]; a car at (x, y) along +x has its circles at x + 1, x, x - 1
    t = hand_track([(20, 20)])
    # the front circle (4.625, -5.125) is 0.375 left of the pixel's left face: penetration 0.5 - 0.375; the others are 1.375 and more away
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(3.625, -5.125, 0.0)]), none, 1, False), row(0.125, 0, 1, 0))
    # the front circle (4.75, -5.5) is (0.25, 0.25) off the pixel's lower left corner (5, -5.25)
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(3.75, -5.5, 0.0)]), none, 1, False), row(0.5 - math.sqrt(0.125), 0, 1, 0))
    # ... and (0.375, 0.375) off it: sqrt(0.28125) > 0.5, nothing
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(3.625, -5.625, 0.0)]), none, 1, False), row(0, 0, 0, 0))
    # the middle circle's centre inside the wall pixel: distance 0, penetration = the radius; front and rear are 0.875 from its faces
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(5.125, -5.125, 0.0)]), none, 1, False), row(0.5, 0, 1, 0))
    # straddling it: front (5.5, .) 0.25 right of the right face, middle (4.5, .) 0.5 left of the left face -- d2 == r*r does not touch
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(4.5, -5.125, 0.0)]), none, 1, False), row(0.25, 0, 1, 0))
    # a softener (body (1, 1), radius 0.25) at (4.875, -5.125), 0.125 from the left face; the chassis circles are 0.875 below the pixel
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(3.875, -6.125, 0.0)]), none, 1, True), row(0.125, 0, 1, 0))
    np.testing.assert_array_equal(cm.contact_rows(t, v, poses([(3.875, -6.125, 0.0)]), none, 1, False), row(0, 0, 0, 0))
    # a wall pixel in the first column, (0, 20) = [0, 0.25] x [-5.25, -5]: the rear circle's centre (-0.125, .) is off the image and
    # touches nothing, 0.125 from the pixel as it is; a quarter unit further in, its centre lies inside the pixel
    t0 = hand_track([(0, 20)])
    np.testing.assert_array_equal(cm.contact_rows(t0, v, poses([(0.875, -5.125, 0.0)]), none, 1, False), row(0, 0, 0, 0))
    np.testing.assert_array_equal(cm.contact_rows(t0, v, poses([(1.125, -5.125, 0.0)]), none, 1, False), row(0.5, 0, 1, 0))
    # two cars nose to tail on an empty map: A's front circle at 4, B's rear circle at 4.75 -- one pair, overlap 1 - 0.75
    empty = hand_track([])
    np.testing.assert_array_equal(cm.contact_rows(empty, v, poses([(3.0, -3.0, 0.0), (5.75, -3.0, 0.0)]), [0, 0], 2, False),
                                  np.array([[0, 0.25, 0, 1], [0, 0.25, 0, 1]], dtype=f))
    # ... in two envs of one car each they are no mates
    assert not cm.contact_rows(empty, v, poses([(3.0, -3.0, 0.0), (5.75, -3.0, 0.0)]), [0, 0], 1, False).any()
    # coincident cars: equal circles coincide (d2 == 0 is left out), the others are 1 or 2 apart (d2 == r2*r2 does not count)
    assert not cm.contact_rows(empty, v, poses([(3.0, -3.0, 0.0), (3.0, -3.0, 0.0)]), [0, 0], 2, False).any()
    assert not cm.contact_rows(empty, v, poses([(3.0, -3.0, 0.0), (4.0, -3.0, 0.0)]), [0, 0], 2, False).any()
    # half a unit apart: five pairs at distance 0.5 -- the mate counts once
    np.testing.assert_array_equal(cm.contact_rows(empty, v, poses([(3.0, -3.0, 0.0), (3.5, -3.0, 0.0)]), [0, 0], 2, False),
                                  np.array([[0, 0.5, 0, 1], [0, 0.5, 0, 1]], dtype=f))
    # three cars in a heap next to a wall pixel, (12, 12) = [3, 3.25] x [-3.25, -3]: every middle circle's centre lies inside it
    heap, tw = poses([(3.0, -3.125, 0.0), (3.5, -3.125, 0.0), (3.25, -3.125, 0.0)]), hand_track([(12, 12)])
    np.testing.assert_array_equal(cm.contact_rows(tw, v, heap, [0, 0, 0], 3, False),
                                  np.array([[0.5, 0.75, 1, 2], [0.25, 0.75, 1, 2], [0.5, 0.75, 1, 2]], dtype=f))
    # the car in the middle slot has finished: its row is zero and nobody counts it as a mate
    np.testing.assert_array_equal(cm.contact_rows(tw, v, heap, [0, 1, 0], 3, False),
                                  np.array([[0.5, 0.75, 1, 1], [0, 0, 0, 0], [0.5, 0.75, 1, 1]], dtype=f))
    np.testing.assert_array_equal(cm.contact_rows(tw, v, heap, [1, 1, 0], 3, False),
                                  np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0.5, 0, 1, 0]], dtype=f))
    rows = cm.contact_rows(tw, v, heap, [0, 0, 0], 3, False)
    assert rows.dtype == f and rows.shape == (3, 4)


# ------------------------------------------------------------------------------------- against the two independent binary64 models
def brute_wall_pens(t, v, pose, bubble, finished):
    """Per car, in the manner of `wall_contact_model` (cos / sin of the yaw, np.clip and np.hypot over ALL wall pixels): the deepest
    r - hypot(...) over the car's circles, how many circles touch, and how close the car comes to a comparison boundary."""
    wall = t.wall_mask()
    sx, sy, ox, oy = t.px_size_x, t.px_size_y, t.origin_x, t.origin_y
    cy, cx = np.nonzero(wall)
    x0, y1 = ox + cx * sx, oy - cy * sy
    x1, y0 = x0 + sx, y1 - sy
    n, yaw = len(pose), TW.yaw_of(pose)
    deepest, touch, margin = np.zeros(n), np.zeros(n, dtype=int), np.full(n, np.inf)
    for i in range(n):
        if finished[i]:
            continue
        c, s = math.cos(yaw[i]), math.sin(yaw[i])
        for bx, by, r in TW.circles_of(v, bubble):
            px, py = pose[i, 0] + c * bx - s * by, pose[i, 1] + s * bx + c * by
            u, w = (px - ox) / sx, (oy - py) / sy
            margin[i] = min(margin[i], abs(u - round(u)), abs(w - round(w)))          # in pixels: which window the centre falls into
            if not (0 <= math.floor(u) < t.width and 0 <= math.floor(w) < t.height):
                continue
            pen = r - np.hypot(px - np.clip(px, x0, x1), py - np.clip(py, y0, y1))
            if len(pen) == 0:
                continue
            margin[i] = min(margin[i], np.abs(pen).min())                              # d2 against r*r
            if pen.max() > 0.0:
                touch[i] += 1
                deepest[i] = max(deepest[i], pen.max())
    return deepest, touch, margin


def brute_car_pens(v, pos, yaw, cpe):
    """Per car, in the manner of `contact_model`: the deepest 2 r - hypot(e) over mates and circle pairs, and the margin to a boundary."""
    n, cx, r2 = len(pos), np.array(list(v.contact_x)), 2.0 * v.contact_radius
    deepest, margin = np.zeros(n), np.full(n, np.inf)
    for i in range(n):
        first = i - i % cpe
        for m in range(first, first + cpe):
            if m == i:
                continue
            for a in cx:
                for b in cx:
                    e = pos[i] + np.array([np.cos(yaw[i]) * a, np.sin(yaw[i]) * a]) - pos[m] - np.array([np.cos(yaw[m]) * b, np.sin(yaw[m]) * b])
                    d = np.hypot(e[0], e[1])
                    margin[i] = min(margin[i], abs(r2 - d), d)
                    if 0.0 < d < r2:
                        deepest[i] = max(deepest[i], r2 - d)
    return deepest, margin


def leave_out(scene, margin, n):
    """The cars on a comparison boundary, named; at most TIED_CAP of the scene."""
    tied = margin < BOUNDARY
    for i in np.nonzero(tied)[0]:
        print(f"{scene}: car {i} sits on a comparison boundary (margin {margin[i]:.2e}) and is left out")
    assert tied.sum() <= TIED_CAP * n, f"{scene}: {int(tied.sum())} of {n} cars on a comparison boundary"
    return ~tied


@pytest.mark.parametrize("name", WALL_SCENES)
def test_wall_rows_meet_the_wall_contact_model(oracle, name):
    sc = TW.contact_scene(name)
    t, v = sc.tracks[0], TW.vehicle_of(oracle, sc)
    with TW.contact_env(oracle, sc, sc.tracks) as e:           # the oracle only brings the scene about: finishers, normalised quaternions
        TW.prepare(e, sc)
        pose, done = e.pose(), e.progress()[:, 4] != 0
    n = len(pose)
    _, touch, _, _, _ = TW.wall_contact_model(t, t.wall_mask(), v, pose, sc.bubble, sc.dt, done)
    deepest, touch2, margin = brute_wall_pens(t, v, pose, sc.bubble, done)
    np.testing.assert_array_equal(touch2, touch)                # the penetrations below are that model's
    rows, _ = cm.contact_rows64(t, v, pose, done, sc.cpe, sc.bubble)
    keep = leave_out(name, margin, n)
    bound = CONTACT_RTOL * np.maximum(deepest, v.contact_radius)
    dev = np.abs(rows[:, cm.WALL_PEN] - deepest)
    print(f"{name}: {n} cars, {int(done.sum())} finished, {int((touch > 0).sum())} touch a wall, {int(touch.sum())} circles; "
          f"worst |pen - model| {dev[keep].max():.2e} (bound {bound.min():.2e} .. {bound.max():.2e}), smallest margin {margin.min():.2e}")
    np.testing.assert_array_equal(rows[keep, cm.WALL_COUNT], touch[keep])
    assert (dev[keep] <= bound[keep]).all(), f"{name}: car {int(np.argmax(dev * keep))}"
    assert (touch > 0).sum() >= 0.25 * (n - done.sum())
    assert not rows[done].any() and (not sc.finish or done.sum() == 5)
    assert (rows[:, cm.WALL_COUNT] <= (7 if sc.bubble else 3)).all() and ((rows[:, cm.WALL_PEN] > 0) <= (rows[:, cm.WALL_COUNT] > 0)).all()
    if sc.bubble:
        assert rows[:, cm.WALL_COUNT].max() > 3


@pytest.mark.parametrize("scene", CPU_PILE_UPS, ids=TC.scene_id)
def test_car_rows_meet_the_car_contact_model(oracle, scene):
    cpe, R, half_width, n_envs, seed = scene
    v, t = oracle.default_vehicle(), open_field()
    pos, yaw = TC.thrown(cpe, half_width, n_envs, seed)
    with capi.Env(oracle, t, n_envs=n_envs, cars_per_env=cpe, n_rays=8) as e:
        pose = e.pose()
        pose[:, 0:2] = pos
        pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
        pose[:, 7:] = 0.0
        e.set_pose(pose)
        pose = e.pose()
    n = len(pose)
    rows, mates = cm.contact_rows64(t, v, pose, np.zeros(n), cpe, False)
    want = np.zeros((n, cpe), dtype=bool)
    for env in range(n_envs):                                   # the model env by env: touching[slot, mate slot] > 0
        a = slice(env * cpe, (env + 1) * cpe)
        want[a] = TC.contact_model(v, pos[a], yaw[a], cpe)[1] > 0
    deepest, margin = brute_car_pens(v, pos, yaw, cpe)
    keep = leave_out(TC.scene_id(scene), margin, n)
    bound = CONTACT_RTOL * np.maximum(deepest, v.contact_radius)
    dev = np.abs(rows[:, cm.CAR_PEN] - deepest)
    print(f"{TC.scene_id(scene)}: {int(want.any(axis=1).sum())} of {n} cars overlap a mate, most mates {int(want.sum(axis=1).max())}; "
          f"worst |pen - model| {dev[keep].max():.2e} (bound {bound.min():.2e} .. {bound.max():.2e}), smallest margin {margin.min():.2e}")
    np.testing.assert_array_equal(mates[keep], want[keep])
    np.testing.assert_array_equal(rows[keep, cm.CAR_COUNT], want[keep].sum(axis=1))
    assert (dev[keep] <= bound[keep]).all()
    assert not rows[:, [cm.WALL_PEN, cm.WALL_COUNT]].any()
    assert 4 * want.any(axis=1).sum() >= n
    if cpe > 2:
        assert (rows[:, cm.CAR_COUNT] >= 2).any()


# ---------------------------------------------------------------------------------------------------------------------- GPU
run_child = functools.partial(children.run_child, CHILD, timeout=300)          # this module's child script and time limit


@pytest.mark.gpu
@pytest.mark.parametrize("name", WALL_SCENES + ["two-tracks"])
def test_gpu_static_wall_scenes_bit_for_bit(name):
    assert "static ok" in run_child("static", scene=name)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", GPU_PILE_UPS, ids=TC.scene_id)
def test_gpu_static_pile_ups_bit_for_bit(scene):
    assert "static ok" in run_child("static", pile_up=scene)


@pytest.mark.gpu
def test_gpu_static_mixed_roster_only_agent_rows_leave():
    assert "static ok" in run_child("static", pile_up=[3, 36, 0.3, 40, 503], roster=["agent", "nidc", "agent"])


@pytest.mark.gpu
def test_twin_walls_both_terminations_both_penalties():
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=64, terminate_on_wall=True, terminate_on_car=True, wall_penalty=1.5,
                    car_penalty=0.75, push="walls", max_episode_steps=150, calls=300, need=["wall_term", "wall_penalised", "final_wall"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_roster_car_terminations_action_repeat_2():
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=8, roster=["agent", "nidc", "agent"], action_repeat=2,
                    terminate_on_car=True, push="cars", max_episode_steps=150, calls=300, need=["car_term", "final_car"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_contacts_with_every_other_signal():
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=64, pool=4, M=6.0, state=True, terminate_off_track=True,
                    off_track_penalty=0.5, terminate_on_wall=True, wall_penalty=1.0, car_penalty=0.25, cars_per_env=2, push="both",
                    max_episode_steps=150, calls=300,
                    need=["wall_term", "off_term", "wall_penalised", "car_penalised", "final_wall", "final_car"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_without_auto_reset_charges_the_penalty_every_call():
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=8, terminate_on_wall=True, wall_penalty=2.0, auto_reset=False,
                    push="walls", max_episode_steps=100, calls=200, need=["wall_term", "wall_penalised"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_two_tracks():
    out = run_child("twin", track=["small-circle", "circle"], envs_per_track=[48, 16], n_envs=64, n_rays=8, terminate_on_wall=True,
                    wall_penalty=0.5, push="walls", max_episode_steps=150, calls=300, need=["wall_term", "wall_penalised", "final_wall"],
                    need_wall_term_per_track=True)
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_on_a_side_stream():
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=8, terminate_on_wall=True, terminate_on_car=True, wall_penalty=1.5,
                    car_penalty=0.75, cars_per_env=2, push="both", side_stream=True, max_episode_steps=100, calls=200,
                    need=["wall_term", "car_term", "wall_penalised", "car_penalised", "final_wall", "final_car"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_contacts_off_is_the_old_call():
    assert "off ok" in run_child("off", calls=200)


@pytest.mark.gpu
def test_all_zero_struct_writes_rows_and_changes_nothing_else():
    assert "zero ok" in run_child("zero", calls=200)


@pytest.mark.gpu
def test_contact_errors():
    assert "errors ok" in run_child("errors")
