"""Signals of the device step (include/ftgp.h: ftgp_device_io_signals / ftgp_step_device_ex / ftgp_state_device /
ftgp_get_centre_dist2; ft_grandprix_amd/vec.py: DeviceVecEnv(scan_pool=, scan_max_range=, state=, terminate_off_track=,
off_track_penalty=)).

GPU: every scenario runs in a fresh child process (tests/device_signals_child.py) that imports torch before libftgp.so is loaded, one
at a time, each under a time limit; a failing child fails its test and is not run again (tests/children.py).  A DeviceVecEnv with signals is compared, bit
for bit at every call, with a numpy model of the header's specification (tests/signals_model.py) fed from the host read-backs of a
twin handle.  CPU: the binding, the argument checks, the model on hand-written rows, and the fixture map the GPU scenario relies on.
"""
import functools
import os

import numpy as np
import pytest

from tests import children
from tests import signals_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "device_signals_child.py")


run_child = functools.partial(children.run_child, CHILD, timeout=600)          # this module's child script and time limit


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_signal_entries():
    import ctypes as C
    from ft_grandprix_amd import capi
    assert C.sizeof(capi.FtgpDeviceSignals) == 16 and capi.FtgpDeviceSignals.off_track_penalty.offset == 12
    assert C.sizeof(capi.FtgpDeviceStepExtra) == 16 and capi.FtgpDeviceStepExtra.final_state.offset == 8
    assert capi.STATE_FLOATS == sm.STATE_FLOATS == len(capi.STATE_FIELDS) == 8
    lib = capi.load()
    for name in ("device_io_signals", "step_device_ex", "state_device", "get_centre_dist2"):
        assert name in capi.API_SYMBOLS and lib.has(name), name


@pytest.mark.parametrize("kwargs", [dict(scan_pool=7), dict(scan_pool=0), dict(scan_pool=-4), dict(scan_pool=128),
                                    dict(scan_max_range=-1.0), dict(scan_max_range=float("nan")), dict(scan_max_range=float("inf")),
                                    dict(off_track_penalty=float("nan")), dict(off_track_penalty=-0.5),
                                    dict(off_track_penalty=float("inf"))])
def test_device_vec_env_checks_the_signals_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import capi, vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, **kwargs)


def test_pool_scan_on_hand_written_rows():
    f = np.float32
    row = np.array([[-1, -1, -1, -1,   -1, 2.5, -1, 0.75,   7.0, 6.0, 9.5, 5.5,   0, 0, 0, 0]], dtype=f)
    # raw: no hit is left out; a beam without any hit is -1
    np.testing.assert_array_equal(sm.pool_scan(row, 4, 0), np.array([[-1, 0.75, 5.5, 0]], dtype=f))
    # clipped at 5 and scaled with inv = float32(1) / float32(5): no hit = the max range, so is everything above it
    inv = f(1.0) / f(5.0)
    np.testing.assert_array_equal(sm.pool_scan(row, 4, 5.0), np.array([[f(5.0) * inv, f(0.75) * inv, f(5.0) * inv, 0]], dtype=f))
    assert sm.pool_scan(row, 4, 5.0).dtype == f and sm.pool_scan(row, 4, 0).dtype == f
    # one beam per ray: raw is the identity, clipped is the scaling alone
    np.testing.assert_array_equal(sm.pool_scan(row, 1, 0), row)
    want = np.array([[5, 5, 5, 5, 5, 2.5, 5, 0.75, 5, 5, 5, 5, 0, 0, 0, 0]], dtype=f) * inv
    np.testing.assert_array_equal(sm.pool_scan(row, 1, 5.0), want)
    # the product, not the quotient: with M = 3 they differ for some range
    r = np.arange(1, 3000, dtype=f)[None, :] / f(1000.0)
    prod = sm.pool_scan(r, 1, 3.0)
    np.testing.assert_array_equal(prod, np.minimum(r, f(3.0)) * (f(1.0) / f(3.0)))
    assert (prod != np.minimum(r, f(3.0)) / f(3.0)).any()
    # an all-zero row (a finished car, an env just reset) stays zero; leading dimensions are kept
    z = np.zeros((2, 3, 12), dtype=f)
    assert sm.pool_scan(z, 3, 0).shape == (2, 3, 4) and not sm.pool_scan(z, 3, 0).any() and not sm.pool_scan(z, 3, 8.0).any()
    assert sm.beam_classes(row, 4, 5.0) == (1, 1, 4) and sm.beam_classes(row, 4, 0) == (1, 1, 0)


def test_state_rows_on_hand_written_records():
    pose = np.zeros((2, 13))
    a = 0.5
    pose[0, [3, 6]] = np.cos(a / 2), np.sin(a / 2)
    pose[0, [7, 8, 12]] = 2.0 * np.cos(a), 2.0 * np.sin(a), 0.25          # rolling along its heading at 2
    pose[1, 3] = 1.0
    pose[1, [7, 8, 12]] = 0.0, -1.5, -0.5                                   # heading +x, sliding towards -y
    ctrl = np.array([[1.5, -0.25], [0.0, 0.0]])
    prog = np.zeros((2, 10), dtype=np.int32)
    prog[0, 2], prog[1, 2], prog[1, 5] = 37, -12, 1
    s = sm.state_rows(pose, ctrl, prog, np.array([0.09, 2.25]))
    assert s.dtype == np.float32 and s.shape == (2, 8)
    np.testing.assert_allclose(s[0], [2.0, 0.0, 0.25, 1.5, -0.25, 0.3, 0.37, 0.0], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(s[1], np.array([0.0, -1.5, -0.5, 0.0, 0.0, 1.5, np.float32(-12 / 100.0), 1.0], dtype=np.float32))


FIXTURE_SHAPES = [(120, 8), (1080, 10), (90, 3)]


@pytest.fixture(scope="module")
def open_right_scans(oracle):
    """The scans of 16 cars on the open-right map after 400 steps straight ahead at speed 3 (the CPU oracle), once for all shapes; and
    the step at which each car of that drive is first off_track, within 1200 steps."""
    from ft_grandprix_amd import capi
    t = sm.open_right_track()
    assert (t.width, t.height, t.px_size_x, t.origin_x, t.origin_y) == (240, 240, 20.0 / 240, -10.0, 10.0)
    wall = t.wall_mask()
    assert wall[:, :3].all() and wall[:3].all() and wall[-3:].all() and not wall[3:-3, 3:].any()
    scans = {}
    ctrl = np.tile(np.array([3.0, 0.0]), (16, 1))
    for n_rays, _ in FIXTURE_SHAPES:
        with capi.Env(oracle, t, n_envs=16, n_rays=n_rays, spawn_mode=1, seed=7) as e:
            e.set_ctrl(ctrl)
            e.step(400)
            scans[n_rays] = e.lidar()
    first_off = np.full(16, -1)
    with capi.Env(oracle, t, n_envs=16, n_rays=4, spawn_mode=1, seed=7) as e:
        e.set_ctrl(ctrl)
        for block in range(12):
            e.step(100)
            off = e.progress()[:, 5] != 0
            first_off[(first_off < 0) & off] = 100 * (block + 1)
    return scans, first_off


@pytest.mark.parametrize("n_rays,pool", FIXTURE_SHAPES)
def test_open_right_map_holds_every_class_of_beam(open_right_scans, n_rays, pool):
    mixed, all_miss, clipped = sm.beam_classes(open_right_scans[0][n_rays], pool, 5.0)
    print(f"{n_rays} / {pool}: {mixed} mixed beams, {all_miss} all-miss beams, {clipped} ranges above 5.0, max {open_right_scans[0][n_rays].max()}")
    assert mixed > 0 and all_miss > 0 and clipped > 0
    assert 5.0 < open_right_scans[0][n_rays].max() < 20.0 * np.sqrt(2) + 1


def test_open_right_map_lets_straight_drivers_leave_the_track(open_right_scans):
    first_off = open_right_scans[1]
    print("first off_track by step", first_off.tolist())
    assert (first_off > 0).all() and first_off.min() >= 500          # nobody before step 400, where the scans are taken; all by 1200


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_twin_open_right_every_signal():
    out = run_child("twin", track="open-right", n_envs=64, n_rays=120, pool=8, M=5.0, terminate_off_track=True, penalty=2.5,
                    max_episode_steps=200, calls=600, need=["off_term", "fin_term", "trunc", "clipped", "mixed", "all_miss"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_roster_raw_pool_10():
    out = run_child("twin", track="small-circle", n_envs=64, roster=["agent", "nidc", "agent"], n_rays=1080, pool=10, M=0.0,
                    action_repeat=2, max_episode_steps=150, calls=300, need=["fin_term", "trunc"])
    assert "twin ok" in out


@pytest.mark.gpu
@pytest.mark.parametrize("pool", [3, 1])
def test_twin_90_rays_without_float4(pool):
    out = run_child("twin", track="small-circle", n_envs=64, n_rays=90, pool=pool, M=8.0, terminate_off_track=True, penalty=1.0,
                    max_episode_steps=150, calls=300, need=["off_term", "trunc", "clipped"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_two_tracks():
    out = run_child("twin", track=["small-circle", "circle"], envs_per_track=[48, 16], n_envs=64, n_rays=64, pool=4, M=6.0,
                    terminate_off_track=True, penalty=0.5, max_episode_steps=150, calls=300, need=["off_term", "trunc"],
                    need_off_term_per_track=True)
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_without_auto_reset_charges_the_penalty_every_call():
    out = run_child("twin", track="open-right", n_envs=64, n_rays=120, pool=8, M=5.0, terminate_off_track=True, penalty=2.5,
                    auto_reset=False, max_episode_steps=100, calls=200, need=["off_term", "trunc"])
    assert "twin ok" in out


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays,pool", [(128, 64), (96, 2), (256, 4), (6400, 32), (8192, 32)])
def test_twin_other_pooling_paths(n_rays, pool):
    """A wave per beam (pool >= 64); whole beams in a lane's float4 (pool 2 and 4); rows staged in more than one chunk of 128 beams:
    6400 rays are a whole chunk and one of 72 beams, 8192 rays two whole chunks (the step kernel's LDS holds one car's fan and
    scans up to some 8700 rays, so longer rows cannot be made)."""
    out = run_child("twin", track="small-circle", n_envs=8 if n_rays > 1000 else 64, n_rays=n_rays, pool=pool, M=8.0, max_episode_steps=40,
                    calls=60, need=["trunc"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_default_signals_are_the_old_call():
    assert "defaults ok" in run_child("defaults", calls=200)


@pytest.mark.gpu
def test_twin_on_a_side_stream():
    out = run_child("twin", track="open-right", n_envs=64, n_rays=120, pool=8, M=5.0, terminate_off_track=True, penalty=2.5,
                    side_stream=True, max_episode_steps=100, calls=200, need=["off_term", "trunc"])
    assert "twin ok" in out


@pytest.mark.gpu
def test_signal_errors():
    assert "errors ok" in run_child("errors")
