"""Per-car vehicle dynamics (include/ftgp.h: FTGP_DYN_DOUBLES, ftgp_set_dynamics / ftgp_set_dynamics_device / ftgp_get_dynamics;
ft_grandprix_amd/vec.py: DeviceVecEnv(randomize_dynamics=, dynamics_seed=)).

CPU: the binding and the argument checks of DeviceVecEnv, which run before the library is loaded.

GPU: every scenario runs in a fresh child process (tests/dynamics_child.py) that imports torch before libftgp.so is loaded, one at a
time, each under a time limit (tests/children.py).  The criterion throughout: car a of a handle with the table on equals, bit for bit,
car a of a CPU-oracle twin without a table whose vehicle carries row a's eight values -- same operations, same order, no tolerance.
Test rows are base * default_rng(seed).uniform(lo, hi, (n, 8)) with the lo / hi of tests/dynamics_child.py.
"""
import functools
import os

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "dynamics_child.py")
ENTRIES = ("set_dynamics", "set_dynamics_device", "get_dynamics")

run_child = functools.partial(children.run_child, CHILD, timeout=300)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_dynamics_entries():
    from ft_grandprix_amd import capi
    assert capi.DYN_DOUBLES == len(capi.DYN_FIELDS) == 8
    assert capi.DYN_FIELDS == ("mass", "izz", "friction", "tire_damping", "throttle_kv", "throttle_force_limit", "steer_kp", "steer_damping")
    assert all(hasattr(capi.FtgpVehicle, f) for f in capi.DYN_FIELDS)
    lib = capi.load()
    for name in ENTRIES:
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None, name
    for method in ("set_dynamics", "set_dynamics_device", "dynamics"):
        assert callable(getattr(capi.Env, method))
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "#define FTGP_DYN_DOUBLES 8" in header and "#define FTGP_ABI_VERSION 5" in header
    for name in ENTRIES:
        assert f"int ftgp_{name}(FtgpEnv *env" in header, name


@pytest.mark.parametrize("bounds", [{"grip": (0.3, 0.9)}, {"friction": (0.9, 0.3)}, {"friction": (0.3, float("inf"))},
                                    {"mass": (float("nan"), 8.0)}, {"mass": (0.0, 8.0)}, {"izz": (-0.01, 0.05)},
                                    {"friction": (-0.1, 0.9)}, {"steer_kp": (-1.0, 20.0)}, {"friction": 0.5}, ["friction"]])
def test_device_vec_env_checks_the_dynamics_bounds_before_a_handle_exists(bounds, monkeypatch):
    from ft_grandprix_amd import capi, vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, randomize_dynamics=bounds)


def test_device_vec_env_accepts_valid_dynamics_bounds_up_to_the_load(monkeypatch):
    from ft_grandprix_amd import capi, vec

    class Reached(Exception):
        pass

    def no_load():
        raise Reached()
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(Reached):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, randomize_dynamics={"friction": (0.3, 0.9), "mass": (4.0, 4.0), "steer_damping": (0.0, 0.5)})


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_closed_loop_matches_the_oracle_twins():
    """19 envs of one car on small-circle, rollout("fast") in three launches of 100 steps: every env equals its oracle twin after each."""
    assert "closed loop ok" in run_child("closed_loop")


@pytest.mark.gpu
@pytest.mark.parametrize("cars_per_env,bubble_wrap", [(3, False), (6, False), (3, True)])
def test_multi_car_envs_match_the_oracle_twins(cars_per_env, bubble_wrap):
    """One row per env, shared by its cars: the one-env oracle twin matches bit for bit, contacts included."""
    assert "multi car ok" in run_child("multi_car", cars_per_env=cars_per_env, bubble_wrap=bubble_wrap)


@pytest.mark.gpu
@pytest.mark.parametrize("cars", [3, 8])
def test_distinct_rows_per_car(cars):
    """One env on an open field, every car its own row; the cars stay at least 0.5 apart, so car a equals car a of the twin whose whole
    env has row a."""
    assert "distinct rows ok" in run_child("distinct_rows", cars=cars)


@pytest.mark.gpu
def test_neutral_rows_reproduce_the_plain_kernel():
    assert "neutral ok" in run_child("neutral")


@pytest.mark.gpu
def test_device_setter():
    assert "device setter ok" in run_child("device_setter")


@pytest.mark.gpu
def test_multi_track_handle():
    assert "multitrack ok" in run_child("multitrack")


@pytest.mark.gpu
def test_tricycle():
    assert "tricycle ok" in run_child("tricycle")


@pytest.mark.gpu
def test_errors():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_device_vec_env_randomises_at_episode_starts():
    assert "vec env ok" in run_child("vec_env")
