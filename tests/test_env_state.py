"""Env states on the device (include/ftgp.h: ftgp_env_state_bytes / ftgp_save_envs_device / ftgp_load_envs_device /
ftgp_get_env_state_rejected / ftgp_obs_device; ft_grandprix_amd/vec.py: DeviceVecEnv.save_state / load_state / fork).

CPU: the binding, the record's layout and the argument checks of DeviceVecEnv, which run before any call into the library.

GPU: every scenario runs in a fresh child process (tests/env_state_child.py) that imports torch before libftgp.so is loaded, one at a
time, each under a time limit (tests/children.py).  The criterion throughout is bit for bit, no tolerance: a handle that saves, runs
on, loads and runs on again equals a twin that was never interrupted in every read-back (pose, progress, lap_times, race_steps, ctrl,
steps, lidar, centre_dist2, winners, episodes, dynamics), and its two legs equal each other.
"""
import contextlib
import functools
import os
import types

import numpy as np
import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "env_state_child.py")
ENTRIES = ("env_state_bytes", "save_envs_device", "load_envs_device", "get_env_state_rejected", "obs_device")

run_child = functools.partial(children.run_child, CHILD, timeout=300)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_env_state_entries():
    from ft_grandprix_amd import capi
    lib = capi.load()
    for name in ENTRIES:
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None and len(lib.fn(name).argtypes) >= 2, name
    for method in ("env_state_bytes", "save_envs_device", "load_envs_device", "env_state_rejected", "obs_device"):
        assert callable(getattr(capi.Env, method))
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "#define FTGP_ABI_VERSION 5" in header and "#define FTGP_ENV_STATE_VERSION 1" in header
    assert capi.ABI_VERSION == 5 and capi.ENV_STATE_VERSION == 1
    assert "#define FTGP_ENV_STATE_MAGIC 0x53454746u" in header and capi.ENV_STATE_MAGIC == 0x53454746
    assert f"#define FTGP_DYN_RECORD {capi.DYN_RECORD}" in header
    assert "int ftgp_env_state_bytes(FtgpEnv *env, size_t *bytes_per_env);" in header
    assert "int ftgp_save_envs_device(FtgpEnv *env, void *stream, void *rows, int64_t n_rows, const uint8_t *env_mask);" in header
    assert "int ftgp_load_envs_device(FtgpEnv *env, void *stream, const void *rows, int64_t n_rows, const int32_t *src_row);" in header
    assert "int ftgp_get_env_state_rejected(FtgpEnv *env, int64_t *rejected);" in header
    assert "int ftgp_obs_device(FtgpEnv *env, void *stream, float *obs);" in header


@pytest.mark.parametrize("n_rays", [8, 90, 1080])
@pytest.mark.parametrize("cars", [1, 3, 8])
def test_env_state_layout_is_aligned(n_rays, cars):
    from ft_grandprix_amd import capi
    lay = capi.env_state_layout(n_rays, cars)
    for part in ("header", "steps", "cars", "dyn", "ranges"):
        assert lay[part] % 16 == 0, (part, lay)
    for stride in ("car_bytes", "dyn_bytes", "row_bytes", "bytes"):
        assert lay[stride] % 16 == 0, (stride, lay)
    assert lay["header"] == 0 and lay["steps"] == 32 and lay["episodes"] == 40 and lay["cars"] == 48
    assert lay["car_bytes"] == 448 and lay["dyn_bytes"] == 8 * capi.DYN_RECORD == 96 and 4 * n_rays <= lay["row_bytes"] < 4 * n_rays + 16
    assert lay["dyn"] == 48 + 448 * cars and lay["ranges"] == lay["dyn"] + 96 * cars
    assert lay["bytes"] == lay["ranges"] + cars * lay["row_bytes"]
    if (n_rays, cars) == (1080, 1):
        assert lay["bytes"] == 4912


def test_unpack_env_state_reads_what_the_layout_says():
    from ft_grandprix_amd import capi
    R, c, n = 90, 3, 4
    lay = capi.env_state_layout(R, c)
    rng = np.random.default_rng(2)
    buf = np.zeros((n, lay["bytes"]), dtype=np.uint8)
    head = np.zeros(n, dtype=capi.ENV_STATE_HEADER_DTYPE)
    head["magic"], head["version"], head["n_rays"], head["cars_per_env"] = capi.ENV_STATE_MAGIC, 1, R, c
    head["fingerprint"] = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    head["steps"], head["episodes"] = rng.integers(0, 2 ** 40, n), rng.integers(0, 99, n)
    buf[:, :48] = head.view(np.uint8).reshape(n, 48)
    cars = np.zeros((n, c), dtype=capi.CAR_STATE_DTYPE)
    for name in capi.CAR_STATE_FIELDS:
        kind = cars.dtype[name].base.kind
        cars[name] = rng.normal(size=cars[name].shape) if kind == "f" else rng.integers(-5, 1000, cars[name].shape)
    buf[:, lay["cars"]:lay["dyn"]] = cars.view(np.uint8).reshape(n, -1)
    dyn = rng.uniform(0.1, 9.0, (n, c, capi.DYN_RECORD))
    buf[:, lay["dyn"]:lay["ranges"]] = dyn.view(np.uint8).reshape(n, -1)
    rows = np.zeros((n, c, lay["row_bytes"] // 4), dtype=np.float32)
    rows[:, :, :R] = rng.uniform(0, 20, (n, c, R))
    buf[:, lay["ranges"]:] = rows.view(np.uint8).reshape(n, -1)
    u = capi.unpack_env_state(buf, R, c)
    for name in capi.ENV_STATE_HEADER_DTYPE.names:
        np.testing.assert_array_equal(u[name], head[name], err_msg=name)
    for name in capi.CAR_STATE_FIELDS:
        np.testing.assert_array_equal(u[name], cars[name], err_msg=name)
    np.testing.assert_array_equal(u["dyn"], dyn)
    np.testing.assert_array_equal(u["ranges"], rows[:, :, :R])
    one = capi.unpack_env_state(buf[2], R, c)
    assert one["steps"].shape == (1,) and one["x"].shape == (1, c) and one["times"].shape == (1, c, capi.MAX_LAP_TIMES)
    np.testing.assert_array_equal(one["ranges"][0], rows[2, :, :R])
    with pytest.raises(ValueError):
        capi.unpack_env_state(buf[:, :-16], R, c)
    # byte offsets of the car record the header documents
    d = capi.CAR_STATE_DTYPE
    assert d.fields["completion"][1] == 136 and d.fields["start"][1] == 168 and d.fields["times"][1] == 192 and d.fields["qs"][1] == 56


def test_track_fingerprint_depends_on_every_part():
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    t = load_track("small-circle")
    base = capi.track_fingerprint(t)
    assert 0 <= base < 2 ** 64 and base == capi.track_fingerprint(load_track("small-circle")) != capi.track_fingerprint(load_track("circle"))
    bits, path = t.bits.copy(), t.path.copy()
    bits[t.height // 2, 0] ^= 1
    path[99, 1] = np.nextafter(path[99, 1], np.inf)
    assert capi.track_fingerprint(types.SimpleNamespace(width=t.width, height=t.height, bits=bits, path=t.path)) != base
    assert capi.track_fingerprint(types.SimpleNamespace(width=t.width, height=t.height, bits=t.bits, path=path)) != base
    assert capi.track_fingerprint(types.SimpleNamespace(width=t.width, height=t.height, bits=t.bits, path=t.path)) == base


def _bare_vec_env(monkeypatch, n_envs=4, n_rays=64, cars=1):
    """A DeviceVecEnv without a handle: what the argument checks of save_state / load_state read, on the CPU; any call into the library
    fails the test."""
    import torch
    from ft_grandprix_amd import capi, vec

    def no_load():
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)

    class NoEnv:
        def __getattr__(self, name):
            raise AssertionError(f"Env.{name} was reached before the arguments were checked")
    v = vec.DeviceVecEnv.__new__(vec.DeviceVecEnv)
    v.n_envs, v.n_rays, v.cars_per_env, v.device, v.env = n_envs, n_rays, cars, torch.device("cpu"), NoEnv()
    v.bytes_per_env = capi.env_state_layout(n_rays, cars)["bytes"]
    v.dynamics, v._dyn_lo = None, None
    v._device_guard, v._stream = contextlib.nullcontext, lambda: 0          # (no GPU here)
    return v, vec, torch


def test_device_vec_env_checks_the_state_arguments_before_any_call(monkeypatch):
    v, vec, torch = _bare_vec_env(monkeypatch)
    good = vec.EnvSnapshot(torch.zeros((4, v.bytes_per_env), dtype=torch.uint8))
    assert good.bytes_per_env == v.bytes_per_env
    bad_snaps = [None, torch.zeros((4, v.bytes_per_env), dtype=torch.uint8),
                 vec.EnvSnapshot(torch.zeros((4, v.bytes_per_env + 16), dtype=torch.uint8)),        # another env's records
                 vec.EnvSnapshot(torch.zeros((4, v.bytes_per_env), dtype=torch.int8)),
                 vec.EnvSnapshot(torch.zeros(4 * v.bytes_per_env, dtype=torch.uint8)),
                 vec.EnvSnapshot(torch.zeros((3, v.bytes_per_env), dtype=torch.uint8)),             # fewer rows than envs, no src
                 vec.EnvSnapshot(torch.zeros((4, 2 * v.bytes_per_env), dtype=torch.uint8)[:, ::2]),
                 vec.EnvSnapshot(torch.zeros((4, v.bytes_per_env), dtype=torch.uint8, device="meta")),
                 vec.EnvSnapshot(torch.zeros((4, v.bytes_per_env), dtype=torch.uint8), dynamics=torch.zeros((4, 2, 8), dtype=torch.float64))]
    for snap in bad_snaps:
        with pytest.raises(ValueError):
            v.load_state(snap)
    bad_src = [[0, 1, 2, 3], torch.zeros(3, dtype=torch.int64), torch.zeros((4, 1), dtype=torch.int64), torch.zeros(4, dtype=torch.float32),
               torch.zeros(4, dtype=torch.int16), torch.zeros(8, dtype=torch.int32)[::2], torch.zeros(4, dtype=torch.int32, device="meta")]
    for src in bad_src:
        with pytest.raises(ValueError):
            v.load_state(good, src)
        with pytest.raises(ValueError):
            v.fork(src)
    bad_mask = [[1, 0, 1, 0], torch.zeros(3, dtype=torch.bool), torch.zeros(4, dtype=torch.int32), torch.zeros(8, dtype=torch.uint8)[::2],
                torch.zeros(4, dtype=torch.bool, device="meta")]
    for mask in bad_mask:
        with pytest.raises(ValueError):
            v.save_state(mask)
    with pytest.raises(ValueError):
        v.save_state(None, out=vec.EnvSnapshot(torch.zeros((3, v.bytes_per_env), dtype=torch.uint8)))
    with pytest.raises(ValueError):
        v.save_state(None, out=torch.zeros((4, v.bytes_per_env), dtype=torch.uint8))


def test_device_vec_env_reaches_the_library_with_valid_state_arguments(monkeypatch):
    """The positive control of the test above: valid arguments get as far as the first call into the library."""
    v, vec, torch = _bare_vec_env(monkeypatch)
    good = vec.EnvSnapshot(torch.zeros((6, v.bytes_per_env), dtype=torch.uint8))
    for call in (lambda: v.load_state(good), lambda: v.load_state(good, torch.tensor([5, -1, 0, 0])),
                 lambda: v.load_state(good, torch.tensor([5, -1, 0, 0], dtype=torch.int32)),
                 lambda: v.save_state(torch.ones(4, dtype=torch.bool)), lambda: v.save_state(torch.ones(4, dtype=torch.uint8), out=good)):
        with pytest.raises(AssertionError, match="was reached before the arguments were checked"):
            call()


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_layout_matches_the_read_backs():
    """19 envs x 3 cars x 90 rays (a scan row that is no multiple of 16 bytes), 150 steps of fast: unpack_env_state of the saved rows
    equals the read-backs field by field."""
    assert "layout ok" in run_child("layout")


@pytest.mark.gpu
@pytest.mark.parametrize("case,policy", [("one_car_1080", "fast"), ("one_car_1080", "nidc"), ("eight_cars", "per_car"), ("bubble_wrap", "per_car"),
                                         ("tricycle", "host"), ("fakelidar", "nidc")])
def test_restore_equals_the_uninterrupted_run(case, policy):
    assert "restore ok" in run_child("restore", case=case, policy=policy)


@pytest.mark.gpu
@pytest.mark.parametrize("lap_target", [5, 1])
def test_restore_across_a_lap_crossing_and_a_finish(lap_target):
    assert "laps ok" in run_child("laps", lap_target=lap_target)


@pytest.mark.gpu
def test_masked_save_and_selective_load():
    assert "masked ok" in run_child("masked")


@pytest.mark.gpu
@pytest.mark.parametrize("cars", [1, 3])
def test_fork(cars):
    assert "fork ok" in run_child("fork", cars=cars)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "auto_reset", "random_start", "dynamics"])
def test_device_vec_env_load_state_repeats_the_calls(case):
    assert "vec env ok" in run_child("vec_env", case=case)


@pytest.mark.gpu
def test_cross_handle_and_multi_track():
    assert "cross ok" in run_child("cross")


@pytest.mark.gpu
def test_errors():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_a_handle_that_never_saves_launches_what_it_launched():
    assert "neutral ok" in run_child("neutral")
