"""Rival rows, race place and the place reward of the device step (include/ftgp.h: FTGP_RIVAL_FIXED, ftgp_device_io_rivals /
ftgp_step_device_rivals / ftgp_rivals_device / ftgp_get_rivals; ft_grandprix_amd/vec.py: DeviceVecEnv(rivals=, n_rivals=,
place_reward=)).

CPU: the binding, the argument checks, the numpy model of the header's text (tests/rival_model.py: `rival_rows64`) on hand-written envs
with exact expected rows, that model against the independent one (`independent_rows`: places from sorted key tuples, mates from a
stable argsort on np.hypot, rotations by -yaw through np.cos / np.sin of arctan2-derived angles) on the four bundled tracks, and the
place-reward arithmetic.

   Scenes: 200 envs per track and per env size (2, 5 and 8 cars), seeded: every car at a random place along the path -- a random point,
   a random way towards the next one -- moved sideways by up to 0.9 of the room the start table leaves on that side, with a random yaw,
   random velocities, a random absolute completion around its lap position, and one car in eight finished.  Every entry must agree within
   1e-12 * max(1, |value|) (the frame test's bound: each entry is at most about six roundings of quantities below 60, so the error is
   under 1e-13), mate order and place exactly, no pose left out.

GPU: every scenario runs in a fresh child process (tests/device_rivals_child.py) that imports torch before libftgp.so is loaded, one at
a time, each under a time limit (tests/children.py).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from ft_grandprix_amd import capi
from tests import children
from tests import frame_model as fm
from tests import rival_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "device_rivals_child.py")
BUNDLED = ["small-circle", "circle", "track", "inkscape"]
RTOL = 1e-12                                                         # the issue's
ENTRIES = ("device_io_rivals", "step_device_rivals", "rivals_device", "get_rivals")


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_rival_entries():
    assert C.sizeof(capi.FtgpDeviceRivals) == 16
    assert [getattr(capi.FtgpDeviceRivals, f).offset for f in ("n_rivals", "reserved", "place_weight", "reserved_f")] == [0, 4, 8, 12]
    assert C.sizeof(capi.FtgpDeviceStepRivals) == 16 and capi.FtgpDeviceStepRivals.rival.offset == 0 and capi.FtgpDeviceStepRivals.final_rival.offset == 8
    assert capi.RIVAL_FIXED == rm.RIVAL_FIXED == len(capi.RIVAL_FIELDS) == 4
    assert capi.RIVAL_FLOATS == rm.RIVAL_FLOATS == len(capi.RIVAL_MATE_FIELDS) == 8 and capi.MAX_RIVALS == rm.MAX_RIVALS == 7
    assert capi.RIVAL_FIELDS == ("place", "n_racing", "gap_ahead", "gap_behind")
    assert capi.RIVAL_MATE_FIELDS == ("fwd", "left", "cos_rel", "sin_rel", "v_fwd", "v_left", "track_gap", "present")
    lib = capi.load()
    for name in ENTRIES:
        assert name in capi.API_SYMBOLS and lib.has(name), name
    for method in ENTRIES:
        assert callable(getattr(capi.Env, method))
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for line in ("#define FTGP_RIVAL_FIXED 4", "#define FTGP_RIVAL_FLOATS 8", "#define FTGP_MAX_RIVALS 7", "#define FTGP_ABI_VERSION 5"):
        assert line in header, line


@pytest.mark.parametrize("kwargs", [dict(n_rivals=-1), dict(n_rivals=8), dict(place_reward=-0.5), dict(place_reward=float("nan")),
                                    dict(place_reward=float("inf"))])
def test_device_vec_env_checks_the_rival_arguments_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, cars_per_env=2, **kwargs)


Z8 = [0.0] * 8
# (scene, n_rivals, {slot: the expected row}, {slot: its mates in order}): every product, sum and difference below is exact
HAND = [
    ("alone", 2, {0: [1, 1, 0, 0] + Z8 + Z8}, {0: []}),
    # a mate dead ahead and dead behind: s = 6.5 and 10.5, g = 6.5 and 10.5
    ("ahead and behind", 1, {0: [2, 2, 4, 0, 2, 0, 1, 0, 0.5, 0.25, 4, 1], 1: [1, 2, 0, 4, -2, 0, 1, 0, -0.5, -0.25, -4, 1]}, {0: [1], 1: [0]}),
    # the car looks west, its mate half a unit south of it is to its left; both at s = 6.5 with absolute completion 6: equal g, slot 0 leads
    ("left, looking west, equal g", 1, {0: [1, 2, 0, 0, 0, 0.5, -1, 0, -2, -1, 0, 1], 1: [2, 2, 0, 0, 0, 0.5, -1, 0, -2, -1, 0, 1]}, {0: [1], 1: [0]}),
    # slots 0 and 2 one unit behind and ahead of slot 1: equal d2, the smaller slot first
    ("equal d2", 2, {1: [2, 3, 2, 2, -1, 0, 1, 0, 0, 0, -2, 1, 1, 0, 1, 0, 0, 0, 2, 1], 0: [3, 3, 2, 0, 1, 0, 1, 0, 0, 0, 2, 1, 2, 0, 1, 0, 0, 0, 4, 1]},
     {1: [0, 2], 0: [1, 2], 2: [1, 0]}),
    ("one spot", 1, {0: [1, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], 1: [2, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]}, {0: [1], 1: [0]}),
    # s = 99.5 with c = 0 (f = -0.5, g = 99.5) against s = 0.25 (g = 100.25): the track gap is +0.75 one way and -0.75 the other
    ("across the line", 1, {0: [2, 2, 0.75, 0, 0.125, -0.25, 1, 0, 0, 0, 0.75, 1], 1: [1, 2, 0, 0.75, -0.125, 0.25, 1, 0, 0, 0, -0.75, 1]}, {0: [1], 1: [0]}),
    # s = 10 against s = 60: +50 wraps to -50, and -50 stays
    ("half a lap apart", 1, {0: [2, 2, 50, 0, 2.5, 12.5, 1, 0, 0, 0, -50, 1], 1: [1, 2, 0, 50, -2.5, -12.5, 1, 0, 0, 0, -50, 1]}, {0: [1], 1: [0]}),
    # the mate two units off the centre-line: f = 0, g = 6 against 6.5; still a mate, at the same s
    ("off-track mate", 1, {0: [1, 2, 0, 0.5, 0, -2, 1, 0, 0, 0, 0, 1], 1: [2, 2, 0.5, 0, 0, 2, 1, 0, 0, 0, 0, 1]}, {0: [1], 1: [0]}),
    # slots 1, 3 and 4 have finished at steps 100, 100 and 90: places 2, 3 and 1, ghosts to the two that race; a finished car has no mates
    ("finishers", 2, {0: [4, 2, 0, 2, -1, 0, 1, 0, 0, 0, -2, 1] + Z8, 2: [5, 2, 2, 0, 1, 0, 1, 0, 0, 0, 2, 1] + Z8, 1: [2, 2, 0, 0] + Z8 + Z8,
                      3: [3, 2, 0, 0] + Z8 + Z8, 4: [1, 2, 0, 0] + Z8 + Z8}, {0: [2], 2: [0], 1: [], 3: [], 4: []}),
    # n_rivals 7 with 3 cars: two mates and five slots of zeros; n_rivals 0: the fixed entries alone
    ("equal d2", 7, {1: [2, 3, 2, 2, -1, 0, 1, 0, 0, 0, -2, 1, 1, 0, 1, 0, 0, 0, 2, 1] + Z8 * 5}, {1: [0, 2]}),
    ("equal d2", 0, {0: [3, 3, 2, 0], 1: [2, 3, 2, 2], 2: [1, 3, 0, 2]}, {}),
]


@pytest.mark.parametrize("scene,n_rivals,want,order", HAND, ids=[f"{h[0]}, {h[1]} slots" for h in HAND])
def test_header_model_on_hand_written_envs(scene, n_rivals, want, order):
    cars = rm.hand_scenes()[scene]
    pose, ab, fin, fs = rm.scene_arrays(cars)
    rows64, g, place, mates = rm.rival_rows64(fm.square_path(), pose, ab, fin, fs, len(cars), n_rivals)
    rows = rm.rival_rows(fm.square_path(), pose, ab, fin, fs, len(cars), n_rivals)
    assert rows.dtype == np.float32 and rows.shape == (len(cars), 4 + 8 * n_rivals)
    np.testing.assert_array_equal(rows, rows64.astype(np.float32))
    for slot, row in want.items():
        np.testing.assert_array_equal(rows[slot], np.array(row, dtype=np.float32), err_msg=f"{scene}: slot {slot}")
        assert place[slot] == row[0]
    for slot, m in order.items():
        assert mates[slot].tolist() == m + [-1] * (7 - len(m)), f"{scene}: mates of slot {slot}"


def test_a_finished_cars_place_is_its_winners_place():
    """ftgp_get_winners hands out places by (finish_step, car index) among the finishers of an env."""
    cars = rm.hand_scenes()["finishers"]
    pose, ab, fin, fs = rm.scene_arrays(cars)
    _, _, place, _ = rm.rival_rows64(fm.square_path(), pose, ab, fin, fs, len(cars), 0)
    finishers = sorted((int(fs[k]), k) for k in range(len(cars)) if fin[k])
    for rank, (_, k) in enumerate(finishers):
        assert place[k] == rank + 1


def bundled_scene(name, cpe, n_envs=200, seed=0):
    """Random envs along a bundled track, inside the start table's clearance: (path, pose, absolute_completion, finished, finish_step)."""
    from ft_grandprix_amd.track import load_track
    from tests import spawn_model as sp
    t = load_track(name)
    table = sp.start_table(t)
    rng = np.random.default_rng([seed, cpe, BUNDLED.index(name)])
    n = n_envs * cpe
    p, w = rng.integers(100, size=n), rng.uniform(size=n)
    x, y, qw, qz, left, right = table[p].T
    nxt = table[(p + 1) % 100]
    sh, ch = 2.0 * (qw * qz), 1.0 - 2.0 * (qz * qz)
    lat = rng.uniform(-0.9, 0.9, size=n)
    lat = lat * np.where(lat >= 0, np.minimum(left, nxt[:, 4]), np.minimum(right, nxt[:, 5]))
    yaw = rng.uniform(-np.pi, np.pi, size=n)
    pose = np.zeros((n, 13))
    pose[:, 0], pose[:, 1] = x + w * (nxt[:, 0] - x) + lat * -sh, y + w * (nxt[:, 1] - y) + lat * ch
    pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    pose[:, 7:9] = rng.uniform(-4.0, 4.0, size=(n, 2))
    ab = (p + 100 * rng.integers(0, 2, size=n) - rng.integers(0, 30, size=n)).astype(np.int32)
    fin = (rng.uniform(size=n) < 0.125).astype(np.int32)
    fs = rng.integers(50, 60, size=n).astype(np.int64)                 # few values: equal finish steps inside an env happen
    return np.asarray(t.path, dtype=np.float64), pose, ab, fin, fs


@pytest.mark.parametrize("name", BUNDLED)
def test_header_model_meets_the_independent_model(name):
    seen = dict(ahead=0, behind=0, left=0, right=0, wrapped=0, places=set(), finished_mates=0, padded=0)
    for cpe in (2, 5, 8):
        path, pose, ab, fin, fs = bundled_scene(name, cpe)
        rows, g, place, mates = rm.rival_rows64(path, pose, ab, fin, fs, cpe, 7)
        want, want_place, want_mates = rm.independent_rows(path, pose, ab, fin, fs, cpe, 7)
        np.testing.assert_array_equal(place, want_place, err_msg=f"{name}, {cpe} cars: place")
        np.testing.assert_array_equal(mates, want_mates, err_msg=f"{name}, {cpe} cars: mate order")
        err = np.abs(rows - want)
        bound = RTOL * np.maximum(1.0, np.abs(want))
        print(f"{name}, {cpe} cars: worst error {err.max():.2e}, worst error / bound {(err / bound).max():.2e}")
        assert (err <= bound).all(), f"{name}, {cpe} cars: rows {np.nonzero((err > bound).any(axis=1))[0][:5]}"
        m = rows[:, 4:].reshape(len(rows), 7, 8)
        there = m[:, :, rm.PRESENT] == 1.0
        seen["ahead"] += int((m[:, :, rm.FWD][there] > 0).sum()); seen["behind"] += int((m[:, :, rm.FWD][there] < 0).sum())
        seen["left"] += int((m[:, :, rm.LEFT][there] > 0).sum()); seen["right"] += int((m[:, :, rm.LEFT][there] < 0).sum())
        _, s, _, _ = rm.progress64(path, pose, ab)
        s = s.reshape(-1, cpe)
        seen["wrapped"] += int((np.abs(s[:, :, None] - s[:, None, :]) >= 50.0).sum())
        seen["places"] |= set(place.tolist())
        seen["padded"] += int((~there).sum())
        assert (there.sum(axis=1) == np.where(fin != 0, 0, (fin.reshape(-1, cpe) == 0).sum(axis=1).repeat(cpe) - 1)).all()
    print(f"{name}: {seen}")
    assert min(seen["ahead"], seen["behind"], seen["left"], seen["right"], seen["wrapped"], seen["padded"]) > 0
    assert seen["places"] == set(range(1, 9))


def test_place_term_arithmetic():
    f = np.float32
    # multiply, then add: w * gained is rounded to binary32 before it meets the reward, which shows in the last bit
    w, r = 0.1, np.array([1.1, 0.3, -1.25, 2.0], dtype=f)
    p0, p1 = np.array([4, 1, 3, 2]), np.array([1, 4, 3, 1])
    fin0 = np.array([0, 0, 0, 1], dtype=bool)
    term = rm.place_term(w, p0, p1, fin0)
    assert term.dtype == f
    np.testing.assert_array_equal(term, np.array([f(w) * f(3), f(w) * f(-3), 0, 0], dtype=f))
    got = rm.place_reward(r, w, p0, p1, fin0)
    assert got.dtype == f
    np.testing.assert_array_equal(got, np.array([f(f(1.1) + f(f(w) * f(3))), f(f(0.3) + f(f(w) * f(-3))), f(-1.25), f(2.0)], dtype=f))
    fused = f(np.float64(f(w)) * 3.0 + np.float64(f(1.1)))            # one rounding: what a fused multiply-add would give
    assert got[0] != fused
    # frozen for a car that had finished, whatever the places say; w == 0: the input array itself
    assert rm.place_term(0.5, [3], [1], [True])[0] == 0 and rm.place_term(0.5, [3], [1], [False])[0] == 1.0
    assert rm.place_reward(r, 0.0, p0, p1, fin0) is r


# ---------------------------------------------------------------------------------------------------------------------- GPU
run_child = functools.partial(children.run_child, CHILD, timeout=90)          # this module's child script and time limit


@pytest.mark.gpu
@pytest.mark.parametrize("track", ["square", "track"])
def test_gpu_get_rivals_on_set_poses_bit_for_bit(track):
    """1, 7, 9, 32, 33, 65 and 261 cars in envs of 1, 3, 5 and 8; d2 ties, a coincident pair, an off-track mate; n_rivals 0, 1, 3, 7."""
    assert "set poses ok" in run_child("set_poses", track=track)


@pytest.mark.gpu
def test_gpu_finished_cars_are_ghosts_with_their_winners_place():
    assert "finished ok" in run_child("finished")


@pytest.mark.gpu
def test_gpu_closed_loop_rows_place_reward_and_resets():
    assert "closed loop ok" in run_child("closed_loop", calls=120)


@pytest.mark.gpu
def test_gpu_multi_track_rows_follow_each_envs_path():
    assert "multi track ok" in run_child("multi_track")


@pytest.mark.gpu
def test_gpu_rivals_off_is_the_old_call_and_the_error_codes():
    assert "off ok" in run_child("off", calls=80)
