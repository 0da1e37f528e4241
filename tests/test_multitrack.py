"""Multi-track handles (include/ftgp.h: ftgp_create_tracks, ftgp_get_track_distance_field; capi.Env and vec.DeviceVecEnv with a list of
tracks).

CPU: ftgp_create_tracks' argument checks run before the device probe (FTGP_ERR_ARG, never FTGP_ERR_NO_DEVICE, on a machine without a
GPU); the default split and the argument checks of capi.Env and DeviceVecEnv; the binding.
GPU: every scenario runs in a fresh child process (tests/multitrack_child.py) under a time limit (tests/children.py): a four-track handle against one
single-track handle per env block, bit for bit (the matrix of cars per env, rays, lidar modes, spawn modes and policies; masked
resets, set_pose, the metrics record), against the oracle, both workgroup orders, the distance fields and fixture G8, device I/O.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from ft_grandprix_amd import capi
from ft_grandprix_amd.track import load_track
from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "multitrack_child.py")
NAMES = ["track", "circle", "small-circle", "inkscape"]


run_child = functools.partial(children.run_child, CHILD, timeout=600)          # this module's child script and time limit


# ---------------------------------------------------------------------------------------------------------------------- CPU
class Huge:
    """An image whose sector box field would reach 4 GiB (the pattern of test_box_field_must_stay_addressable_with_32_bits): the check
    sits in front of the device probe, the bitmap is never read."""
    width, height = 8192, 8192
    px_size_x = px_size_y = 40.0 / 8192
    origin_x, origin_y = 0.0, 0.0
    bits = np.zeros((1, 256), dtype=np.uint32)
    path = np.zeros((100, 2))


def create_tracks(lib, tracks, counts, n_envs=None, null_tracks=False, null_counts=False, n_tracks=None):
    """ftgp_create_tracks through ctypes, as it lies: (status, error text)."""
    cfg = capi.FtgpConfig()
    cfg.abi_version, cfg.cars_per_env, cfg.n_rays, cfg.lap_target, cfg.dt = capi.ABI_VERSION, 1, 64, 10, 0.004
    cfg.n_envs = int(sum(counts)) if n_envs is None else n_envs
    cfg.vehicle = lib.default_vehicle()
    arr = (capi.FtgpTrack * max(1, len(tracks)))()
    keep = [capi._fill_track(arr[k], t) for k, t in enumerate(tracks)]
    cnt = np.array(list(counts) or [0], dtype=np.int32)
    h = C.c_void_p()
    rc = lib.fn("create_tracks")(C.byref(cfg), None if null_tracks else arr, None if null_counts else cnt.ctypes.data_as(C.c_void_p),
                                 len(tracks) if n_tracks is None else n_tracks, C.byref(h))
    del keep
    if rc == 0:
        lib.fn("destroy")(h)
    return rc, lib.last_error()


@pytest.fixture(scope="module")
def four():
    return [load_track(n) for n in NAMES]


def test_binding_declares_the_multi_track_entries(product):
    assert "create_tracks" in capi.API_SYMBOLS and "get_track_distance_field" in capi.API_SYMBOLS
    assert product.has("create_tracks") and product.has("get_track_distance_field")
    assert capi.MAX_TRACKS == 16
    assert "#define FTGP_MAX_TRACKS 16" in open(os.path.join(ROOT, "include", "ftgp.h")).read()


@pytest.mark.parametrize("n_tracks", [0, 17])
def test_create_tracks_refuses_a_track_count_out_of_range(product, four, n_tracks):
    tracks = (four * 5)[:max(n_tracks, 1)]
    rc, msg = create_tracks(product, tracks, [1] * len(tracks), n_tracks=n_tracks)
    assert rc == -1 and "n_tracks" in msg, (rc, msg)


def test_create_tracks_refuses_an_empty_block(product, four):
    rc, msg = create_tracks(product, four, [3, 0, 2, 1])
    assert rc == -1 and "track 1" in msg, (rc, msg)


def test_create_tracks_refuses_counts_that_do_not_sum_to_n_envs(product, four):
    rc, msg = create_tracks(product, four, [3, 1, 2, 1], n_envs=8)
    assert rc == -1 and "sums to 7" in msg, (rc, msg)


@pytest.mark.parametrize("which", ["tracks", "counts"])
def test_create_tracks_refuses_null_arrays(product, four, which):
    rc, msg = create_tracks(product, four, [1, 1, 1, 1], null_tracks=which == "tracks", null_counts=which == "counts")
    assert rc == -1 and "null" in msg, (rc, msg)


def test_create_tracks_names_the_bad_track(product, four):
    class Bad:
        width, height = 0, 10
        px_size_x = px_size_y = 0.1
        origin_x = origin_y = 0.0
        bits = np.zeros((10, 1), dtype=np.uint32)
        path = np.zeros((100, 2))
    rc, msg = create_tracks(product, [four[0], four[1], Bad, four[3]], [1, 1, 1, 1])
    assert rc == -1 and msg.startswith("track 2: bad track"), (rc, msg)
    rc, msg = create_tracks(product, [four[0], Huge, four[2]], [2, 1, 1])
    assert rc == -1 and msg.startswith("track 1: ") and "4 GiB" in msg, (rc, msg)


def test_create_tracks_checks_every_track_before_the_device(product, four):
    class NoPixels:
        width, height = 64, 64
        px_size_x, px_size_y = 0.1, 0.0
        origin_x = origin_y = 0.0
        bits = np.zeros((64, 2), dtype=np.uint32)
        path = np.zeros((100, 2))
    rc, msg = create_tracks(product, four + [NoPixels], [1, 1, 1, 1, 1])
    assert rc == -1 and msg.startswith("track 4: bad dt / pixel size"), (rc, msg)


def test_env_splits_envs_evenly_with_the_remainder_first():
    assert capi.split_envs(10, 4) == (3, 3, 2, 2)
    assert capi.split_envs(4096, 4) == (1024,) * 4
    assert capi.split_envs(5, 5) == (1,) * 5
    assert capi.track_blocks(9, 2) == (5, 4)
    assert capi.track_blocks(9, 2, [2, 7]) == (2, 7)


@pytest.mark.parametrize("n_envs, n_tracks, counts", [(3, 4, None), (8, 0, None), (40, 17, None), (8, 2, [4, 3]), (8, 2, [8, 0]),
                                                      (8, 2, [4, 2, 2])])
def test_env_checks_the_blocks(n_envs, n_tracks, counts):
    with pytest.raises(ValueError):
        capi.track_blocks(n_envs, n_tracks, counts)


def test_env_checks_the_blocks_before_a_handle_exists(four):
    class NoLib:
        def fn(self, name):
            raise AssertionError("the library was called before the blocks were checked")
    with pytest.raises(ValueError):
        capi.Env(NoLib(), four, n_envs=8, envs_per_track=[1, 2, 3])
    with pytest.raises(ValueError):
        capi.Env(NoLib(), four[0], n_envs=8, envs_per_track=[8])


@pytest.mark.parametrize("kwargs", [dict(track=[]), dict(track=["circle", "nowhere-at-all"]), dict(track=["circle", 3]),
                                    dict(track=NAMES, envs_per_track=[1, 1, 1]), dict(track=NAMES, envs_per_track=[5, 1, 1, 0]),
                                    dict(track="circle", envs_per_track=[7]), dict(track=NAMES * 5)])
def test_device_vec_env_checks_the_tracks_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises((ValueError, KeyError, FileNotFoundError)):
        vec.DeviceVecEnv(n_envs=7, n_rays=64, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("lidar_mode, n_rays, cars_per_env",
                         [(m, r, c) for m in ("rangefinder", "fakelidar") for r in (90, 1080) for c in (1, 3)] +
                         [("rangefinder", 1080, 7), ("fakelidar", 90, 7)],         # crowded envs: env-mates 4 to 6, two envs per workgroup
                         ids=lambda v: str(v))
def test_gpu_four_tracks_equal_the_blocks_bit_for_bit(cars_per_env, n_rays, lidar_mode):
    run_child("equivalence", cars_per_env=cars_per_env, n_rays=n_rays, lidar_mode=lidar_mode, steps=200 if lidar_mode == "rangefinder" else 100)


@pytest.mark.gpu
def test_gpu_four_tracks_match_the_oracle_block_by_block():
    run_child("oracle_blocks")


@pytest.mark.gpu
def test_gpu_one_track_is_ftgp_create():
    run_child("one_track")


@pytest.mark.gpu
def test_gpu_workgroup_orders_agree():
    run_child("orders")


@pytest.mark.gpu
def test_gpu_track_distance_fields_and_g8():
    run_child("distance_fields")


@pytest.mark.gpu
def test_gpu_comm_init_refuses_a_multi_track_handle():
    run_child("comm_refused")


@pytest.mark.gpu
@pytest.mark.parametrize("action_repeat", [1, 2])
def test_gpu_device_io_on_four_tracks_equals_the_blocks(action_repeat):
    run_child("device_io", action_repeat=action_repeat, calls=400 if action_repeat == 1 else 200)
