"""Collected rollouts (include/ftgp.h "Collected rollouts": ftgp_collect_device; ft_grandprix_amd/vec.py: DeviceVecEnv.collect).

CPU: the binding and the header; the argument checks that need no device; the shipped element operations of step 1's noise, clip and
guard (csrc/ftgp_net.h, compiled for the host by tools/collect_check.cpp, also under the address and undefined-behaviour sanitizers)
against the numpy model of the header's text (tests/collect_model.py), bit for bit, and both against edge rows written out by hand.

GPU: every scenario runs in a fresh child process (tests/collect_child.py) that imports torch before libftgp.so is loaded, one at a
time, each under a time limit (tests/children.py).  The criterion throughout is equality to the bit -- with the model, and with a twin
handle stepped one ftgp_step_device_rivals call at a time: no tolerance anywhere.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import children
from tests import collect_model as cmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "collect_child.py")

run_child = functools.partial(children.run_child, CHILD, timeout=300)
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_entry_and_the_header_keeps_its_abi_line():
    from ft_grandprix_amd import capi
    lib = capi.load()
    assert "collect_device" in capi.API_SYMBOLS and lib.has("collect_device")
    assert lib.fn("collect_device").argtypes is not None
    assert callable(capi.Env.collect_device)
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "#define FTGP_ABI_VERSION 5" in header
    assert "int ftgp_collect_device(FtgpEnv *env, const FtgpCollect *c);" in header
    # void*, 2 x int32, 3 x float[2], 9 pointers, int32 and its padding
    assert ctypes.sizeof(capi.FtgpCollect) == 8 + 8 + 24 + 9 * 8 + 8 == 120
    assert capi.FtgpCollect.noise.offset == 40 and capi.FtgpCollect.reset_dynamics.offset == 104 and capi.FtgpCollect.reserved.offset == 112
    for field in ("stream", "slot", "n_decisions", "std", "lo", "hi", "noise", "inputs", "mean", "action", "reward", "terminated", "truncated",
                  "next_inputs", "reset_dynamics", "reserved"):
        assert f" {field}" in header.split("typedef struct FtgpCollect {")[1].split("} FtgpCollect;")[0].replace("*", " "), field


def test_null_arguments_are_refused_without_a_device():
    from ft_grandprix_amd import capi
    lib = capi.load()
    c = capi.collect_args(3)
    assert lib.fn("collect_device")(None, c) == -1 and "null" in lib.last_error()
    assert lib.fn("collect_device")(None, None) == -1


@pytest.mark.parametrize("bad", [dict(n_decisions=0), dict(n_decisions=-1), dict(n_decisions=2.5), dict(n_decisions=2 ** 31), dict(slot=4),
                                 dict(slot=-1), dict(slot="net0"), dict(std=(-0.1, 0.0)), dict(std=(0.0, float("nan"))),
                                 dict(std=(float("inf"), 0.0)), dict(std=(1.0,)), dict(std="x"), dict(clip=((0.0, 1.0),)),
                                 dict(clip=((1.0, 0.0), (0.0, 1.0))), dict(clip=((0.0, 1.0), (0.0, float("inf")))),
                                 dict(clip=((float("nan"), 1.0), (0.0, 1.0)))])
def test_collect_args_refuses_bad_fields_before_a_handle_is_touched(bad):
    from ft_grandprix_amd import capi
    kw = {"n_decisions": 4, **bad}
    with pytest.raises(ValueError):
        capi.collect_args(**kw)


def test_collect_args_fills_the_scalar_fields():
    from ft_grandprix_amd import capi
    c = capi.collect_args(7, 2, (0.5, 0.25), ((0.0, 3.0), (-0.5, 0.5)))
    assert (c.n_decisions, c.slot, c.reserved) == (7, 2, 0)
    assert list(c.std) == [0.5, 0.25] and list(c.lo) == [0.0, -0.5] and list(c.hi) == [3.0, 0.5]
    assert not any((c.stream, c.noise, c.inputs, c.mean, c.action, c.reward, c.terminated, c.truncated, c.next_inputs, c.reset_dynamics))
    lo_is_hi = capi.collect_args(1, clip=((1.0, 1.0), (0.0, 0.0)))
    assert list(lo_is_hi.lo) == list(lo_is_hi.hi) == [1.0, 0.0]


def test_device_vec_env_collect_checks_its_arguments_first():
    """DeviceVecEnv.collect on an object that holds no handle: the refusals come before anything of the env is used."""
    from ft_grandprix_amd import vec
    env = object.__new__(vec.DeviceVecEnv)
    env._nets = {}
    for kw in (dict(n_decisions=0), dict(n_decisions=3, std=(-1.0, 0.0)), dict(n_decisions=3, clip=((2.0, 1.0), (0.0, 1.0))),
               dict(n_decisions=3, slot=5), dict(n_decisions=3)):
        with pytest.raises(ValueError):
            env.collect(**kw)


def sanitizers_available(cxx, flags, tmp):
    """Whether the host compiler builds and runs an empty program with the sanitizer flags: decided before the code under test is touched."""
    src = tmp / "empty.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp / "empty")
    if subprocess.run([cxx, *flags, str(src), "-o", exe], capture_output=True, text=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True, text=True).returncode == 0


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("collect")
    out = str(tmp / f"collect_check_{request.param}")
    flags = ["-O2", "-ffp-contract=off", "-std=c++17"]
    if request.param == "sanitized":
        # (the runtimes linked statically where the compiler knows the switches: the program then needs nothing of its environment)
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]          # (clang links them statically anyway)
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static]
        if not sanitizers_available(cxx, flags, tmp):
            pytest.skip("the host compiler has no sanitizer runtimes (an empty program does not build and run with them)")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "collect_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_harness(harness, tmp_path, name, y, noise, scale, offset, std, lo, hi):
    """(mean, action) float32 [n, 2] of tools/collect_check on the given rows."""
    y, noise = np.ascontiguousarray(y, dtype=F), np.ascontiguousarray(noise, dtype=F)
    src, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([len(y)], dtype=np.int32).tofile(f)
        np.array([*scale, *offset, *std, *lo, *hi], dtype=F).tofile(f)
        y.tofile(f); noise.tofile(f)
    r = subprocess.run([harness, str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=F).reshape(2, len(y), 2)
    return got[0], got[1]


def test_edge_rows_written_out_by_hand(harness, tmp_path):
    """Rows whose results are written down here by hand from the header's text: the shipped element operations (the host harness) and
    the numpy model must both give them."""
    inf, nan = F(np.inf), F(np.nan)
    one, zero = (1.0, 1.0), (0.0, 0.0)                               # an output map that leaves y as it is: mean = fmaf(y, 1, 0)
    m = np.array([[1.0, 0.25], [1.0, 0.25], [1.0, 0.25], [inf, 0.0], [nan, 0.0], [2.0, -inf], [1.0, 0.25], [-0.0, 0.0]], dtype=F)
    z = np.array([[1.0, -1.0], [100.0, -100.0], [inf, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [nan, 0.0], [0.0, 0.0]], dtype=F)

    def both(name, rows, noise, std, lo, hi, want):
        cmod.assert_same_bits(cmod.action(rows, std, noise, lo, hi), want, f"{name}: the model")
        got_m, got_a = run_harness(harness, tmp_path, name, rows, np.zeros_like(rows) if noise is None else noise, one, zero, std, lo, hi)
        cmod.assert_same_bits(got_a, want, f"{name}: the harness")
        cmod.assert_same_bits(got_m, cmod.mean(rows, one, zero), f"{name}: the harness' mean")
    both("plain", m, z, (0.5, 0.25), (0.0, -0.5), (3.0, 0.5),
         [[1.5, 0.0], [3.0, -0.5], [3.0, 0.25],                     # ordinary; both clipped; infinite noise times std > 0: the bound
          [3.0, 0.0], [0.0, 0.0], [2.0, -0.5],                      # an infinite mean becomes the bound; a NaN mean: both 0
          [0.0, 0.0], [0.0, 0.0]])                                  # NaN noise: both 0
    # std = 0 and an infinite draw: 0 * infinity is a NaN, and the guard zeroes BOTH components
    both("std0_inf", m[:1], np.array([[inf, 1.0]], dtype=F), (0.0, 0.25), (0.0, -0.5), (3.0, 0.5), [[0.0, 0.0]])
    # std = 0 and finite draws: the clipped mean
    both("std0", m[:2], z[:2], (0.0, 0.0), (0.0, -0.5), (0.5, 0.5), [[0.5, 0.25]] * 2)
    # lo == hi: that value, unless the sum is a NaN
    both("lo_is_hi", m[[0, 1, 2, 3, 5, 4, 6]], z[[0, 1, 2, 3, 5, 4, 6]], (0.5, 0.25), (1.25, 0.125), (1.25, 0.125), [[1.25, 0.125]] * 5 + [[0.0, 0.0]] * 2)
    # no noise = zeros: fmaf(std, 0, m) = m, and -0 + (+0) = +0
    both("no_noise", m[[0, 7]], None, (0.5, 0.25), (-9.0, -9.0), (9.0, 9.0), [[1.0, 0.25], [0.0, 0.0]])
    # the mean is one fused multiply-add, not guarded: (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24, and a product rounded on its own would have
    # lost the 2^-24
    y = np.array([[F(1.0) + F(2.0 ** -12), 2.0], [inf, nan]], dtype=F)
    scale, offset = (F(1.0) + F(2.0 ** -12), 0.5), (-1.0, 0.25)
    for got in (cmod.mean(y, scale, offset), run_harness(harness, tmp_path, "fma", y, np.zeros_like(y), scale, offset, zero, (-9.0, -9.0), (9.0, 9.0))[0]):
        assert got[0, 0] == F(2.0 ** -11 + 2.0 ** -24) != F(2.0 ** -11) and got[0, 1] == F(1.25)
        assert np.isinf(got[1, 0]) and np.isnan(got[1, 1])
    assert cmod.same_bits([nan, 0.0], [nan, 0.0]) and not cmod.same_bits([0.0], [-0.0]) and not cmod.same_bits([1.0], [nan])


@pytest.mark.parametrize("case", sorted(cmod.element_cases()))
def test_host_harness_equals_the_model(harness, tmp_path, case):
    c = cmod.element_cases()[case]
    y, noise = c["y"], c["noise"]
    assert np.isnan(noise).any() and np.isposinf(noise).any() and np.isneginf(noise).any()
    got_m, got_a = run_harness(harness, tmp_path, case, y, noise, c["scale"], c["offset"], c["std"], c["lo"], c["hi"])
    m = cmod.mean(y, c["scale"], c["offset"])
    a = cmod.action(m, c["std"], noise, c["lo"], c["hi"])
    cmod.assert_same_bits(got_m, m, f"{case}: mean")
    cmod.assert_same_bits(got_a, a, f"{case}: action")
    assert np.isfinite(a).all() and (a == 0).all(axis=1).any() and (a != 0).any()
    assert ((a >= F(c["lo"])) & (a <= F(c["hi"])) | (a == 0).all(axis=1)[:, None]).all()


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_replay_and_model():
    """7 envs x 1 car at 64 rays with the one-layer net; 3 envs x 3 cars [agent, fast, agent] at 1080 rays with mlp_tanh (85 inputs: the
    second input register) and with off_wave: 7 and 6 rows, no multiple of a workgroup's four waves.  T = 12, max_episode_steps = 5,
    auto-reset, random noise, a clip that binds for some rows: inputs, mean and action equal the model on the twin's read-backs,
    reward / terminated / truncated the twin's, and the env-state records of both handles are equal at the end."""
    assert "replay and model ok" in run_child("replay_and_model")


@pytest.mark.gpu
def test_next_inputs_are_the_state_before_the_reset():
    """Signals with the net's pool and max_range, the twin with state and final buffers: next_inputs[t] == inputs[t + 1] for envs not
    reset at t; for reset envs it is the twin's final_obs window joined with final_state[0:5], and inputs[t + 1] holds zero beams and
    the spawn state."""
    assert "next inputs ok" in run_child("next_inputs")


@pytest.mark.gpu
def test_a_collected_agent_moves_like_a_roster_car():
    """action_repeat = 1, no noise, a wide clip, no episode end, T = 20: pose and lidar equal ftgp_rollout(FTGP_POLICY_NET0, 20)."""
    assert "against roster ok" in run_child("against_roster")


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ["contacts", "dense progress", "spawn rule", "two tracks", "action repeat 3", "place reward"])
def test_the_rules_of_the_device_step_ride_along(scenario):
    """One rule each, compared with the twin as in test_replay_and_model: contacts with terminating rules and penalties; the dense
    progress reward; a spawn rule; a two-track handle; action_repeat = 3; the rivals' place reward."""
    assert f"rules {scenario} ok" in run_child("rules", only=scenario)


@pytest.mark.gpu
def test_finished_cars_and_a_diverged_network():
    """lap_target = 0, two agents per env: every row reads mean = action = (0, 0) while the inputs are recorded.  An infinite weight in
    the last layer: where it meets a hidden output of exactly 0 the mean is a NaN in the record and the action is (0, 0); where it meets
    hidden outputs that are not 0 the mean is infinite and, by the written order (the clip, then the guard), the action is the bound."""
    assert "finished and diverged ok" in run_child("finished_and_diverged")


@pytest.mark.gpu
def test_reset_dynamics_follow_the_episode_ends():
    """Envs that end at different decisions: each holds the rows of its last end afterwards, the others are untouched, an invalid row
    is rejected and counted, and everything equals the twin with masked ftgp_set_dynamics_device calls.  FTGP_ERR_STATE without
    auto_reset."""
    assert "reset dynamics ok" in run_child("reset_dynamics")


@pytest.mark.gpu
def test_every_refusal_leaves_the_handle_as_it_was():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_device_vec_env_collect():
    """Shapes, out= reuse, alternation with step() against a twin env, on a non-default torch stream with the noise produced on that
    stream right before the call; noise=True / None; randomize_dynamics keeps its mirror."""
    assert "vec env ok" in run_child("vec_env")
