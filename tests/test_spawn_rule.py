"""The spawn rule (include/ftgp.h: FtgpSpawnRule, ftgp_set_spawn_rule / ftgp_get_episodes / ftgp_get_start_table;
ft_grandprix_amd/vec.py: DeviceVecEnv(random_start=, start_points=, start_margin=, start_lateral=, start_yaw_jitter=, shuffle_grid=)).

CPU: the binding, the argument checks, and the shipped start-table builder and draw (csrc/ftgp_spawn.h, compiled for the host by
tools/spawn_check.cpp) against the numpy model of the header's text (tests/spawn_model.py), bit for bit, on the four bundled tracks.
The model builds the spawn table's quaternions with math.atan2 / cos / sin, the libm the host plan calls, and the whole table --
x, y, qw, qz and both clearances -- is compared bit for bit: feeding the model the harness's columns was not needed.

GPU: every scenario runs in a fresh child process (tests/spawn_rule_child.py) that imports torch before libftgp.so is loaded, one at a
time, each under a time limit.  A child that ends by a signal, an abort or its time limit fails its test, and every later child of
the session is refused (tests/children.py).
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from ft_grandprix_amd import capi
from ft_grandprix_amd.track import load_track
from tests import children
from tests import spawn_model as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "spawn_rule_child.py")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TRACKS = ["track", "circle", "small-circle", "inkscape"]
RULE = sp.Rule(first_point=0, n_points=100, shuffle_grid=True, margin=0.1, lateral_frac=0.8, yaw_tan=math.tan(0.1))
IDENTITY = sp.Rule(first_point=10, n_points=1, shuffle_grid=False, margin=0.0, lateral_frac=0.0, yaw_tan=0.0)
SEED, ENV_BASE, N_ENVS, EPISODES = 7, 3, 64, 4


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_spawn_entries():
    assert C.sizeof(capi.FtgpSpawnRule) == 40
    fields = ("first_point", "n_points", "shuffle_grid", "reserved", "margin", "lateral_frac", "yaw_tan")
    assert [getattr(capi.FtgpSpawnRule, f).offset for f in fields] == [0, 4, 8, 12, 16, 24, 32]
    lib = capi.load()
    for name in ("set_spawn_rule", "get_episodes", "get_start_table"):
        assert name in capi.API_SYMBOLS and lib.has(name), name
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "typedef struct FtgpSpawnRule" in header and "#define FTGP_ABI_VERSION 5" in header and capi.ABI_VERSION == 5


@pytest.mark.parametrize("kwargs", [dict(start_points=(-1, 10)), dict(start_points=(100, 10)), dict(start_points=(0, 0)),
                                    dict(start_points=(0, 101)), dict(start_margin=-0.1), dict(start_margin=float("nan")),
                                    dict(start_margin=float("inf")), dict(start_lateral=-0.01), dict(start_lateral=1.01),
                                    dict(start_lateral=float("nan")), dict(start_yaw_jitter=-0.1), dict(start_yaw_jitter=float("nan")),
                                    dict(start_yaw_jitter=math.pi), dict(start_yaw_jitter=float("inf"))])
def test_device_vec_env_checks_the_start_arguments_before_a_handle_exists(kwargs, monkeypatch):
    from ft_grandprix_amd import vec

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, **kwargs)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("spawn") / "spawn_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tools", "spawn_check.cpp"), "-o", out, "-w"])
    return out


def write_track(t, path):
    with open(path, "wb") as f:
        np.array([t.width, t.height, t.words_per_row, 0], dtype=np.int32).tofile(f)
        np.array([t.px_size_x, t.px_size_y, t.origin_x, t.origin_y], dtype=np.float64).tofile(f)
        np.ascontiguousarray(t.path, dtype=np.float64).tofile(f)
        np.ascontiguousarray(t.bits, dtype=np.uint32).tofile(f)


def run_harness(harness, tmp_path, t, cars, rule, seed=SEED, env_base=ENV_BASE, n_envs=N_ENVS, episodes=EPISODES):
    raw, out = tmp_path / f"{t.name}.raw", tmp_path / f"{t.name}-{cars}.bin"
    write_track(t, raw)
    r = subprocess.run([harness, str(raw), str(out), str(seed), str(env_base), str(n_envs), str(cars), str(episodes), str(rule.first_point),
                        str(rule.n_points), str(int(rule.shuffle_grid)), float(rule.margin).hex(), float(rule.lateral_frac).hex(),
                        float(rule.yaw_tan).hex()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = open(out, "rb").read()
    n = episodes * n_envs * cars
    table = np.frombuffer(blob, dtype=np.float64, count=600).reshape(100, 6)
    n_start = int(np.frombuffer(blob, dtype=np.int32, count=1, offset=4800)[0])
    start = np.frombuffer(blob, dtype=np.int32, count=100, offset=4804)
    pose = np.frombuffer(blob, dtype=np.float64, count=4 * n, offset=5204).reshape(episodes, n_envs, cars, 4)
    draw = np.frombuffer(blob, dtype=np.int32, count=4 * n, offset=5204 + 32 * n).reshape(episodes, n_envs, cars, 4)
    assert len(blob) == 5204 + 48 * n
    return table, start[:n_start].tolist(), pose, draw


_TABLES = {}


def model_table(name):
    if name not in _TABLES:
        _TABLES[name] = sp.start_table(load_track(name))
    return _TABLES[name]


_DRAWS = {}


def model_draws(name, cars, k):
    """The model's draws of the CPU comparison, computed once."""
    key = (name, cars, k)
    if key not in _DRAWS:
        table = model_table(name)
        _DRAWS[key] = sp.draw_batch(SEED, ENV_BASE, N_ENVS, cars, k, RULE, table, load_track(name).path, sp.start_list(table, RULE))
    return _DRAWS[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", TRACKS)
def test_shipped_start_table_and_draw_equal_the_model_bit_for_bit(harness, tmp_path, name):
    t, table = load_track(name), model_table(name)
    start = sp.start_list(table, RULE)
    for cars in (1, 3, 8):
        got_table, got_start, pose, draw = run_harness(harness, tmp_path, t, cars, RULE)
        np.testing.assert_array_equal(bits(got_table[:, :4]), bits(table[:, :4]), err_msg="spawn table (x, y, qw, qz)")
        np.testing.assert_array_equal(bits(got_table[:, 4:]), bits(table[:, 4:]), err_msg="clearances")
        assert got_start == start
        for k in range(EPISODES):
            want = model_draws(name, cars, k)
            at = f"{name}, {cars} cars, episode {k}"
            np.testing.assert_array_equal(draw[k, :, :, 0], want["p"], err_msg="p: " + at)
            np.testing.assert_array_equal(draw[k, :, :, 1], want["slot"], err_msg="slot: " + at)
            np.testing.assert_array_equal(bits(pose[k]), bits(want["pose"]), err_msg="pose: " + at)
            np.testing.assert_array_equal(draw[k, :, :, 2], want["offset"], err_msg="offset: " + at)


def test_the_model_draws_cover_what_the_rule_is_for():
    """Counted on the model's data alone, over the draws the comparison above uses."""
    seen = dict(left=0, right=0, shuffled=0, no_room=0, moved_offset=0, n=0)
    for name in TRACKS:
        table = model_table(name)
        blocked = [p for p in range(100) if min(table[p, 4], table[p, 5]) < RULE.margin]
        print(f"{name}: blocked at margin {RULE.margin}: {blocked}; median clearance {np.median(table[:, 4:]):.3f}, smallest {table[:, 4:].min():.3f}")
        assert blocked == {"track": [69, 70, 71, 72], "circle": [87, 88, 89, 90, 91], "small-circle": [], "inkscape": []}[name]
        assert len(sp.start_list(table, RULE)) == 100 - len(blocked)
        for cars in (1, 3, 8):
            for k in range(EPISODES):
                want = model_draws(name, cars, k)
                seen["left"] += int((want["side"] == sp.LEFT).sum()); seen["right"] += int((want["side"] == sp.RIGHT).sum())
                seen["shuffled"] += int((want["slot"] != np.arange(cars)).any(axis=1).sum())
                seen["no_room"] += int((want["room"] == 0.0).sum())
                seen["moved_offset"] += int((want["offset"] != want["p"]).sum())
                seen["n"] += want["p"].size
                assert (np.sort(want["slot"], axis=1) == np.arange(cars)).all()       # every grid is a permutation
                assert (np.abs(np.hypot(want["pose"][:, :, 2], want["pose"][:, :, 3]) - 1.0) < 1e-15).all()
    print(seen)
    assert seen["left"] > 0 and seen["right"] > 0, "both sides are drawn"
    assert seen["shuffled"] > 0, "a grid that is not the identity"
    assert seen["no_room"] > 0, "a grid mate without room"
    assert seen["moved_offset"] > 0, "a placement whose nearest centre-line point is not its start point"


@pytest.mark.parametrize("name", TRACKS)
def test_identity_rule_gives_spawn_mode_0(name):
    t, table = load_track(name), model_table(name)
    start = sp.start_list(table, IDENTITY)
    assert start == [10]
    for k in (0, 1, 5):
        d = sp.draw_batch(SEED, 0, 4, 3, k, IDENTITY, table, t.path, start)
        np.testing.assert_array_equal(d["p"], np.tile([10, 12, 14], (4, 1)))
        np.testing.assert_array_equal(bits(d["pose"]), bits(np.tile(table[[10, 12, 14], :4], (4, 1, 1))))
        np.testing.assert_array_equal(d["offset"], d["p"])


# ---------------------------------------------------------------------------------------------------------------------- GPU
run_child = functools.partial(children.run_child, CHILD, timeout=300)          # this module's child script and time limit


@pytest.mark.gpu
@pytest.mark.parametrize("cars, n_envs", [(3, 96), (7, 40)])
def test_gpu_resets_equal_the_model_bit_for_bit(cars, n_envs):
    assert "model ok" in run_child("model", cars=cars, n_envs=n_envs)


@pytest.mark.gpu
def test_gpu_identity_rule_is_spawn_mode_0():
    assert "identity ok" in run_child("identity")


@pytest.mark.gpu
def test_gpu_rule_off_is_the_fixed_start_again():
    assert "off ok" in run_child("off")


@pytest.mark.gpu
@pytest.mark.parametrize("signals", [False, True], ids=["finish_kernel", "finish_signals_kernel"])
def test_gpu_auto_reset_follows_the_rule(signals):
    assert "auto_reset ok" in run_child("auto_reset", signals=signals)


@pytest.mark.gpu
def test_gpu_shards_draw_what_the_whole_batch_draws():
    assert "shards ok" in run_child("shards")


@pytest.mark.gpu
def test_gpu_spawn_rule_errors():
    assert "errors ok" in run_child("errors")
