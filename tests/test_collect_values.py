"""Collected rollouts with values (include/ftgp.h "Collected rollouts with values": ftgp_set_value_net, ftgp_collect_values_device,
ftgp_gae_device; ft_grandprix_amd/vec.py: DeviceVecEnv.collect(values=True), gae).

CPU: the binding and the header; the argument checks that need no device; the shipped element step of the advantage scan and the value
element (csrc/ftgp_net.h, compiled for the host by tools/collect_values_check.cpp, also under the address and undefined-behaviour
sanitizers) against the numpy model of the header's text (tests/collect_values_model.py), bit for bit, and both against a row written
out by hand whose advantages are computed in binary64 from the textbook recursion.

GPU: every scenario runs in a fresh child process (tests/collect_values_child.py), one at a time, each under a time limit
(tests/children.py).  The criterion throughout is equality to the bit -- with the model, and with a twin handle that ran plain
ftgp_collect_device: no tolerance anywhere.
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import children
from tests import collect_model as cmod
from tests import collect_values_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "collect_values_child.py")

run_child = functools.partial(children.run_child, CHILD, timeout=300)
F = np.float32
NEW = ("set_value_net", "set_value_net_device", "get_value_net", "collect_values_device", "gae_device")


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_header_binding_and_export_agree():
    from ft_grandprix_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for name in NEW:
        assert name in capi.API_SYMBOLS and lib.has(name) and lib.fn(name).argtypes is not None, name
        assert re.search(r"\bint ftgp_%s\(FtgpEnv \*env" % name, header), name
    assert "#define FTGP_ABI_VERSION 5" in header and capi.ABI_VERSION == 5
    assert ctypes.sizeof(capi.FtgpCollect) == 120
    assert "int ftgp_collect_values_device(FtgpEnv *env, const FtgpCollect *c, const FtgpCollectValues *v);" in header
    # int32, int32[4], 2 x int32, 2 x float, int32
    V = capi.FtgpValueDesc
    assert ctypes.sizeof(V) == 4 + 16 + 8 + 8 + 4 == 40
    assert (V.n_layers.offset, V.width.offset, V.hidden_act.offset, V.out_act.offset, V.out_scale.offset, V.out_offset.offset, V.reserved.offset) == \
        (0, 4, 20, 24, 28, 32, 36)
    # 2 x float, 4 pointers, int32[2]
    W = capi.FtgpCollectValues
    assert ctypes.sizeof(W) == 8 + 4 * 8 + 8 == 48
    assert (W.gamma.offset, W.lam.offset, W.value.offset, W.next_value.offset, W.advantage.offset, W.ret.offset, W.reserved.offset) == (0, 4, 8, 16, 24, 32, 40)
    for struct, names in (("FtgpValueDesc", ("n_layers", "width", "hidden_act", "out_act", "out_scale", "out_offset", "reserved")),
                          ("FtgpCollectValues", ("gamma", "lam", "value", "next_value", "advantage", "ret", "reserved"))):
        body = header.split("typedef struct %s {" % struct)[1].split("} %s;" % struct)[0].replace("*", " ").replace(",", " ").replace(";", " ").replace("[", " ")
        words = body.split()
        order = [words.index(n) for n in names]
        assert order == sorted(order), (struct, order)                  # the fields, in the binding's order
    for name in ("set_value_net", "set_value_net_device", "get_value_net", "collect_values_device", "gae_device"):
        assert callable(getattr(capi.Env, name))


def test_null_handles_are_refused_without_a_device():
    from ft_grandprix_amd import capi
    lib = capi.load()
    d, _ = capi.value_desc([(np.zeros((1, 3)), np.zeros(1))])
    p = np.zeros(4, dtype=F)
    assert lib.fn("set_value_net")(None, 0, d, p.ctypes.data) == -1 and "null" in lib.last_error()
    assert lib.fn("set_value_net_device")(None, None, 0, None) == -1 and "null" in lib.last_error()
    assert lib.fn("get_value_net")(None, 0, None, None) == -1 and "null" in lib.last_error()
    assert lib.fn("collect_values_device")(None, capi.collect_args(3), capi.collect_values_args()) == -1 and "null" in lib.last_error()
    assert lib.fn("collect_values_device")(None, None, None) == -1
    assert lib.fn("gae_device")(None, None, 3, 0.9, 0.9, None, None, None, None, None, None, None) == -1 and "null" in lib.last_error()


def layers_of(*widths):
    return [(np.zeros((o, i), dtype=F), np.zeros(o, dtype=F)) for i, o in zip(widths[:-1], widths[1:])]


@pytest.mark.parametrize("bad", [dict(layers=layers_of(5, 4, 2)), dict(layers=layers_of(5, 2)), dict(layers=layers_of(5, 0, 1)),
                                 dict(layers=layers_of(5, 129, 1)), dict(layers=[]), dict(layers=layers_of(5, 4, 4, 4, 4, 1)),
                                 dict(layers=layers_of(5, 4, 1), hidden_act="gelu"), dict(layers=layers_of(5, 4, 1), out_act=2),
                                 dict(layers=layers_of(5, 4, 1), out_scale=float("inf")), dict(layers=layers_of(5, 4, 1), out_scale=float("nan")),
                                 dict(layers=layers_of(5, 4, 1), out_offset=float("-inf")),
                                 dict(layers=[(np.zeros((4, 5)), np.zeros(4)), (np.zeros((1, 3)), np.zeros(1))])])
def test_value_desc_refuses_bad_fields_before_a_handle_is_touched(bad):
    from ft_grandprix_amd import capi
    with pytest.raises(ValueError):
        capi.value_desc(**bad)


def test_value_desc_fills_the_fields():
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.net import ValueSpec
    rng = np.random.default_rng(1)
    net = vm.random_value_net(rng, (17, 128, 1, 1), hidden_act="relu", out_act="tanh", out_scale=2.5, out_offset=-0.5)
    d, flat = capi.value_desc(net["layers"], **vm.value_fields(net))
    assert (d.n_layers, list(d.width), d.hidden_act, d.out_act, d.out_scale, d.out_offset, d.reserved) == (3, [128, 1, 1, 0], 1, 2, 2.5, -0.5, 0)
    assert flat.dtype == F and flat.size == 128 * 17 + 128 + 128 + 1 + 1 + 1 == capi.value_param_count(d, 17)
    for (W, b), (W2, b2) in zip(net["layers"], capi.value_layers(d, flat, 17)):
        np.testing.assert_array_equal(W, W2); np.testing.assert_array_equal(b, b2)
    spec = ValueSpec(net["layers"], **vm.value_fields(net))
    assert spec.widths == (17, 128, 1, 1) and spec.param_count == flat.size
    np.testing.assert_array_equal(spec.flat_params(), flat)
    again = spec.with_params(flat[::-1].copy())
    assert again.widths == spec.widths and again.fields() == spec.fields()
    np.testing.assert_array_equal(again.flat_params(), flat[::-1])


def test_value_spec_round_trips_through_a_file_and_through_torch(tmp_path):
    import torch.nn as nn
    from ft_grandprix_amd.net import ValueSpec, value_from_torch
    module = nn.Sequential(nn.Linear(17, 32), nn.ReLU(), nn.Linear(32, 8), nn.ReLU(), nn.Linear(8, 1))
    spec = value_from_torch(module, out_scale=3.0, out_offset=0.25)
    assert spec.widths == (17, 32, 8, 1) and (spec.hidden_act, spec.out_act, spec.out_scale, spec.out_offset) == ("relu", "identity", 3.0, 0.25)
    np.testing.assert_array_equal(spec.layers[0][0], module[0].weight.detach().numpy())
    spec.save(tmp_path / "critic.npz")
    back = ValueSpec.load(tmp_path / "critic.npz")
    assert back.widths == spec.widths and back.fields() == spec.fields()
    np.testing.assert_array_equal(back.flat_params(), spec.flat_params())
    for bad in (nn.Sequential(nn.Linear(17, 2)), nn.Sequential(nn.Linear(17, 4), nn.Sigmoid(), nn.Linear(4, 1)), nn.Linear(17, 1),
                nn.Sequential(nn.Linear(17, 4), nn.ReLU(), nn.Linear(4, 4), nn.Tanh(), nn.Linear(4, 1))):
        with pytest.raises((ValueError, TypeError)):
            value_from_torch(bad)


@pytest.mark.parametrize("bad", [dict(gamma=float("nan")), dict(gamma=-0.1), dict(gamma=1.5), dict(lam=float("nan")), dict(lam=-0.1), dict(lam=1.5),
                                 dict(gamma=float("inf")), dict(lam="x"), dict(advantage=4096), dict(ret=4096)])
def test_collect_values_args_refuses_bad_fields_before_a_handle_is_touched(bad):
    from ft_grandprix_amd import capi
    with pytest.raises(ValueError):
        capi.collect_values_args(**{"value": 4096, "next_value": 8192, **bad})


def test_collect_values_args_fills_the_fields():
    from ft_grandprix_amd import capi
    v = capi.collect_values_args(0.99, 0.95, 4096, 8192)
    assert (v.gamma, v.lam) == (float(F(0.99)), float(F(0.95))) and (v.value, v.next_value, v.advantage, v.ret) == (4096, 8192, None, None)
    assert list(v.reserved) == [0, 0]
    v = capi.collect_values_args(0.0, 1.0, 4096, 8192, 12288, 16384)
    assert (v.gamma, v.lam, v.advantage, v.ret) == (0.0, 1.0, 12288, 16384)


def test_device_vec_env_checks_its_value_arguments_first():
    """DeviceVecEnv.collect(values=True) on an object that holds no handle: the refusals come before anything of the env is used."""
    from ft_grandprix_amd import vec
    env = object.__new__(vec.DeviceVecEnv)
    env._nets = {0: (((17, 2),), None)}
    for kw in (dict(gamma=1.5), dict(lam=-0.1), dict(gamma=float("nan")), dict()):       # (the last one: the slot has no value net)
        with pytest.raises(ValueError):
            env.collect(3, values=True, **kw)
    with pytest.raises(TypeError):
        env.collect(3, 0, (0.0, 0.0), ((0.0, 1.0), (0.0, 1.0)), None, False, None, True)      # values is keyword-only
    with pytest.raises(TypeError):
        vec.Rollout(*([None] * 9))                                                        # and so are the new fields of a Rollout
    assert vec.Rollout(*([None] * 6)).advantage is None


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
    tmp = tmp_path_factory.mktemp("collect_values")
    out = str(tmp / f"collect_values_check_{request.param}")
    flags = ["-O2", "-ffp-contract=off", "-std=c++17"]
    if request.param == "sanitized":
        # (the runtimes linked statically where the compiler knows the switches: the program then needs nothing of its environment)
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]          # (clang links them statically anyway)
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static]
        if not sanitizers_available(cxx, flags, tmp):
            pytest.skip("the host compiler has no sanitizer runtimes (an empty program does not build and run with them)")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "collect_values_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_harness(harness, tmp_path, name, case, y=(), scale=1.0, offset=0.0):
    """(advantage, ret, v) of tools/collect_values_check on a case of the scan and on value elements y."""
    r, v, nv = (np.ascontiguousarray(case[k], dtype=F) for k in ("reward", "value", "next_value"))
    te, tr = (np.ascontiguousarray(case[k], dtype=np.uint8) for k in ("terminated", "truncated"))
    y = np.ascontiguousarray(y, dtype=F)
    T, n_envs, n_ext = r.shape
    src, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([T, n_envs, n_ext, y.size], dtype=np.int32).tofile(f)
        np.array([case["gamma"], case["lam"], scale, offset], dtype=F).tofile(f)
        for a in (r, v, nv, te, tr, y):
            a.tofile(f)
    p = subprocess.run([harness, str(src), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.fromfile(out, dtype=F)
    n = r.size
    return got[:n].reshape(r.shape), got[n:2 * n].reshape(r.shape), got[2 * n:]


@pytest.mark.parametrize("case", sorted(vm.scan_cases()))
def test_scan_harness_equals_the_model(harness, tmp_path, case):
    c = vm.scan_cases()[case]
    if case.startswith("random"):
        for k in ("reward", "value"):
            assert np.isnan(c[k]).any() and np.isposinf(c[k]).any() and np.isneginf(c[k]).any()
        assert c["terminated"].any() and c["truncated"].any() and not c["terminated"].all()
    if case == "all_terminated":
        assert c["terminated"].all()
    if case == "truncated_only":
        assert c["truncated"].any() and not c["terminated"].any()
    adv, ret, _ = run_harness(harness, tmp_path, case, c)
    want_adv, want_ret = vm.gae(c["reward"], c["value"], c["next_value"], c["terminated"], c["truncated"], c["gamma"], c["lam"])
    cmod.assert_same_bits(adv, want_adv, f"{case}: advantage")
    cmod.assert_same_bits(ret, want_ret, f"{case}: ret")
    if not case.startswith("random"):
        assert np.isfinite(want_adv).any()
    if case == "all_terminated":                                      # nothing of next_value or of a later step counts
        cmod.assert_same_bits(want_adv, (c["reward"] - c["value"]).astype(F), "all terminated: A = r - V")
    if case == "gamma_0_lam_1":                                       # fmaf(0, nv, r) = r for finite nv, and gl = 0
        ok = np.isfinite(c["next_value"]) & np.isfinite(want_adv)
        assert ok.any()


def test_a_row_written_out_by_hand(harness, tmp_path):
    """gamma = lam = 1/2, powers of two, a termination and a truncation inside T = 6: the advantages of the textbook recursion in
    binary64 are exactly representable, and the model and the shipped element step must both give exactly them."""
    case, A64, R64 = vm.hand_row()
    assert case["terminated"].sum() == 1 and case["truncated"].sum() == 1 and case["reward"].shape == (6, 1, 1)
    assert (A64.astype(F).astype(np.float64) == A64).all() and (R64.astype(F).astype(np.float64) == R64).all()
    np.testing.assert_array_equal(A64.ravel(), [1.3125, -0.75, 1.0, 1.4375, -2.75, 4.25])       # (and written down once more)
    adv, ret = vm.gae(case["reward"], case["value"], case["next_value"], case["terminated"], case["truncated"], 0.5, 0.5)
    cmod.assert_same_bits(adv, A64.astype(F), "the model")
    cmod.assert_same_bits(ret, R64.astype(F), "the model's returns")
    adv, ret, _ = run_harness(harness, tmp_path, "hand", case)
    cmod.assert_same_bits(adv, A64.astype(F), "the harness")
    cmod.assert_same_bits(ret, R64.astype(F), "the harness' returns")


def test_the_value_element_is_one_fused_multiply_add(harness, tmp_path):
    """(1 + 2^-12)^2 - 1 = 2^-11 + 2^-24: a product rounded on its own would have lost the 2^-24.  No guard: infinity and NaN pass."""
    one = F(1.0) + F(2.0 ** -12)
    y = np.array([one, np.inf, np.nan, -0.0], dtype=F)
    case, _, _ = vm.hand_row()
    _, _, v = run_harness(harness, tmp_path, "fma", case, y=y, scale=one, offset=-1.0)
    x = y[:, None]                                                    # the model: a one-layer identity net that hands y through
    net = dict(layers=[(np.ones((1, 1), dtype=F), np.zeros(1, dtype=F))], hidden_act="identity", out_act="identity", out_scale=one, out_offset=-1.0)
    for got in (v, vm.value(net, x)):
        assert got[0] == F(2.0 ** -11 + 2.0 ** -24) != F(2.0 ** -11)
        assert np.isposinf(got[1]) and np.isnan(got[2]) and got[3] == F(-1.0)


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one_layer 7x1", "wide 3x3"])
def test_replay_and_model(shape):
    """7 envs x 1 car at 64 rays, a one-layer policy and a one-layer value net; 3 envs x 3 cars [agent, fast, agent] at 1080 rays with
    the 85-input net and value nets of hidden widths 128, 65 and 1.  T = 12, max_episode_steps = 5, auto-reset, noise, a clip that
    binds: every buffer of c and the env-state records equal a twin that ran plain ftgp_collect_device; value, next_value, advantage
    and ret equal the model; next_value[t] == value[t + 1] where the env did not end, and differs where it did."""
    assert "replay and model ok" in run_child("replay_and_model", only=shape)


@pytest.mark.gpu
def test_bootstrap_without_next_inputs():
    assert "bootstrap ok" in run_child("bootstrap")


@pytest.mark.gpu
def test_gae_device_alone():
    """The crafted rows of the CPU test at 7 and at 130 rows; a collected rollout's own advantage; the rewards scaled by 0.5."""
    assert "gae ok" in run_child("gae")


@pytest.mark.gpu
def test_finished_cars_and_a_diverged_critic():
    assert "finished and diverged ok" in run_child("finished_and_diverged")


@pytest.mark.gpu
def test_refresh_and_clearing():
    assert "refresh ok" in run_child("refresh")


@pytest.mark.gpu
def test_a_population_slot_has_one_critic():
    assert "population ok" in run_child("population")


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ["action repeat 3", "two tracks", "frame and rivals"])
def test_the_rules_ride_along(scenario):
    assert f"rules {scenario} ok" in run_child("rules", only=scenario)


@pytest.mark.gpu
def test_every_refusal_leaves_the_handle_as_it_was():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_device_vec_env_values():
    assert "vec env ok" in run_child("vec_env")
