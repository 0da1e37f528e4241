"""Device I/O (include/ftgp.h: ftgp_device_io_config / ftgp_step_device; ft_grandprix_amd/vec.py: DeviceVecEnv).

Every GPU scenario runs in a fresh child process (tests/device_io_child.py) that imports torch before libftgp.so is loaded -- one
HIP runtime per process (vec.py) -- while this process may already hold the library.  The children run one at a time, each under
a time limit; a failing child fails its test and is not run again (tests/children.py).

GPU: DeviceVecEnv against a twin handle stepped through the host path (set_ctrl + step + get_lidar + reset(mask)), bit for bit at
every call; the roster; FAKELIDAR mode; ordering on a non-default torch stream; auto_reset off; the slot table kept apart from
ftgp_set_car_policies' roster; errors.  CPU: the runtime guard, the argument checks, the binding.
"""
import functools
import os

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "device_io_child.py")


run_child = functools.partial(children.run_child, CHILD, timeout=900)          # this module's child script and time limit


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_runtime_guard_passes_with_torch_first():
    out = run_child("guard", timeout=300, order="torch_first")
    assert "guard passed" in out


def test_runtime_guard_raises_when_the_library_came_first():
    out = run_child("guard", timeout=300, order="lib_first")
    assert "libftgp.so was loaded before torch in this process; start a fresh process" in out


def test_guard_counts_distinct_runtime_files():
    from ft_grandprix_amd import vec
    one = ("7f00-7f01 r-xp 0 08:01 1 /x/torch/lib/libamdhip64.so\n"
           "7f01-7f02 r--p 0 08:01 1 /x/torch/lib/libamdhip64.so\n"
           "7f02-7f03 r-xp 0 08:01 2 /x/torch/lib/libhsa-runtime64.so\n")
    vec.check_single_hip_runtime(one)
    two = one + "7f04-7f05 r-xp 0 08:01 3 /opt/rocm-7.2.0/lib/libamdhip64.so.7.2.70200\n"
    with pytest.raises(RuntimeError, match="start a fresh process"):
        vec.check_single_hip_runtime(two)
    # under rocprofv3 the profiler maps its own HSA runtime beside torch's: one HIP runtime, so that alone passes
    prof = one + ("7f06-7f07 r-xp 0 08:01 4 /opt/rocm-7.2.0/lib/librocprofiler-sdk.so.1.0.0\n"
                  "7f07-7f08 r-xp 0 08:01 5 /opt/rocm-7.2.0/lib/libhsa-runtime64.so.1.18.70200\n")
    vec.check_single_hip_runtime(prof)
    with pytest.raises(RuntimeError, match="two copies of libamdhip64"):
        vec.check_single_hip_runtime(prof + "7f09-7f0a r-xp 0 08:01 6 /opt/rocm-7.2.0/lib/libamdhip64.so.7.2.70200\n")


@pytest.mark.parametrize("kwargs", [dict(roster=["nidc"]), dict(cars_per_env=2, roster=["agent"]), dict(action_repeat=0),
                                    dict(roster=["agent", "pilot"], cars_per_env=2), dict(n_envs=0), dict(cars_per_env=9),
                                    dict(lidar_mode="sonar")])
def test_device_vec_env_checks_arguments_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import capi, vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=kwargs.pop("n_envs", 4), n_rays=64, **kwargs)


def test_binding_declares_the_device_io_entries():
    import ctypes as C
    from ft_grandprix_amd import capi
    assert "device_io_config" in capi.API_SYMBOLS and "step_device" in capi.API_SYMBOLS
    # the structs of include/ftgp.h, field by field
    assert C.sizeof(capi.FtgpDeviceIoConfig) == 24 and capi.FtgpDeviceIoConfig.action_repeat.offset == 16
    assert C.sizeof(capi.FtgpDeviceStep) == 56 and capi.FtgpDeviceStep.final_obs.offset == 48
    lib = capi.load()
    assert lib.has("device_io_config") and lib.has("step_device")


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("repeat", [1, 3])
def test_twin_one_car_bit_for_bit(repeat):
    out = run_child("twin", action_repeat=repeat, calls=1500)
    assert "twin ok" in out


@pytest.mark.gpu
@pytest.mark.parametrize("roster", [["agent", "nidc", "fast"], ["nidc", "agent", "fast"],
                                    ["nidc", "fast", "nidc", "nidc", "agent", "nidc", "agent"]])      # agent slots 4 and 6 of a 7-car env
def test_twin_roster(roster):
    out = run_child("twin", n_envs=128, cars_per_env=len(roster), roster=roster, calls=500, action_repeat=2, max_episode_steps=300)
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_fakelidar():
    out = run_child("twin", n_envs=64, lidar_mode="fakelidar", calls=300, max_episode_steps=150, action_repeat=2)
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_on_a_side_stream():
    out = run_child("twin", side_stream=True, calls=400, max_episode_steps=200)
    assert "twin ok" in out


@pytest.mark.gpu
def test_twin_without_auto_reset():
    out = run_child("twin", auto_reset=False, calls=400, max_episode_steps=200, need_ends=False)
    assert "twin ok" in out


@pytest.mark.gpu
def test_device_io_keeps_the_users_roster():
    assert "shared roster ok" in run_child("shared_roster")


@pytest.mark.gpu
def test_device_io_errors():
    assert "errors ok" in run_child("errors")
