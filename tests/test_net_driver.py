"""Network drivers (include/ftgp.h "Network drivers": ftgp_set_net / ftgp_set_net_device / ftgp_get_net, FTGP_POLICY_NET0 .. NET3;
ft_grandprix_amd/net.py; ft_grandprix_amd/vec.py: DeviceVecEnv(nets=, roster=[..., "net0"]) and set_net).

CPU: the binding; the numpy model's TANH and exact fmaf (tests/net_model.py restates the header's text); the shipped element
operations (csrc/ftgp_net.h, compiled for the host by tools/net_check.cpp) against that model, bit for bit; the argument checks, which
run before the library is loaded; NetSpec round trips.

GPU: every scenario runs in a fresh child process (tests/net_driver_child.py) that imports torch before libftgp.so is loaded, one at a
time, each under a time limit (tests/children.py).  The criterion throughout is equality to the bit with the model, evaluated on the
host and fed to a twin as host controls: no tolerance anywhere.
"""
import functools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import children
from tests import net_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "net_driver_child.py")
ENTRIES = ("set_net", "set_net_device", "get_net")

run_child = functools.partial(children.run_child, CHILD, timeout=300)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_network_entries():
    from ft_grandprix_amd import capi
    lib = capi.load()
    for name in ENTRIES:
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None, name
    for method in ("set_net", "set_net_device", "net"):
        assert callable(getattr(capi.Env, method))
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    assert "#define FTGP_ABI_VERSION 5" in header and "#define FTGP_MAX_NETS 4" in header
    for s in range(4):
        assert capi.POLICY_BY_NAME[f"net{s}"] == 6 + s
        assert any(line.split()[:3] == ["#define", f"FTGP_POLICY_NET{s}", str(6 + s)] for line in header.splitlines()), s
    for name in ENTRIES:
        assert f"int ftgp_{name}(FtgpEnv *env" in header, name
    assert (capi.MAX_NETS, capi.NET_MAX_LAYERS, capi.NET_MAX_INPUTS, capi.NET_MAX_HIDDEN) == (4, 4, 256, 128)
    import ctypes
    assert ctypes.sizeof(capi.FtgpNetDesc) == 4 * 17


def test_model_tanh_stays_within_4e_7_of_tanh():
    x = np.linspace(-12.0, 12.0, 2_000_001).astype(np.float32)
    y = nm.tanh(x)
    assert y.dtype == np.float32
    err = np.abs(y.astype(np.float64) - np.tanh(x.astype(np.float64))).max()
    print("largest distance from tanh:", err)
    assert err <= 4e-7
    assert np.abs(y).max() <= 1.0
    np.testing.assert_array_equal(nm.tanh(-x), -y)                  # odd
    assert nm.tanh(np.float32(0.0)) == 0.0
    assert np.isnan(nm.tanh(np.float32(np.nan)))


def test_model_fmaf_is_exact():
    rng = np.random.default_rng(17)
    n = 4000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
    k = np.arange(n) % 3 == 0                                       # cancelling triples: c = -(a * b) rounded, and a neighbour of it
    c[k] = -(a[k].astype(np.float64) * b[k].astype(np.float64)).astype(np.float32)
    near = np.flatnonzero(k)[::2]
    c[near] = np.nextafter(c[near], np.float32(0.0))
    got = nm.fmaf(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        d = abs(Fraction(float(g)) - exact)
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        dl, dh = abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)
        assert d <= dl and d <= dh, (x, y, z, g)
        if d == dl or d == dh:                                      # a tie: the even mantissa
            assert int(np.float32(g).view(np.int32)) & 1 == 0, (x, y, z, g)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("net") / "net_check")
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(ROOT, "tools", "net_check.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("case", sorted(nm.eval_cases()))
def test_host_harness_equals_the_model(harness, tmp_path, case):
    n_rays, nets = nm.eval_cases()[case]
    rng = np.random.default_rng(23)
    n_cars = 5
    for s, net in enumerate(nets):
        scans = nm.eval_scans(rng, n_cars, n_rays, net["max_range"])
        pose, ctrl = nm.eval_records(rng, n_cars)
        if s == 3:                                                  # a diverged network: an infinite weight in front of an identity output, the guard
            net = dict(net, out_act="identity", layers=[(W.copy(), b.copy()) for W, b in net["layers"]])
            net["layers"][-1][0][1, 0] = np.inf
        flat = np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in net["layers"]]).astype(np.float32)
        widths = [W.shape[0] for W, _ in net["layers"]] + [0] * (4 - len(net["layers"]))
        src, out = tmp_path / f"{case}{s}.in", tmp_path / f"{case}{s}.out"
        with open(src, "wb") as f:
            np.array([n_rays, n_cars, net["pool"], net["beam_first"], net["n_beams"], int(net["use_state"]), len(net["layers"]), *widths,
                      nm.ACT[net["hidden_act"]], nm.ACT[net["out_act"]], flat.size], dtype=np.int32).tofile(f)
            np.array([net["max_range"], *net["out_scale"], *net["out_offset"]], dtype=np.float32).tofile(f)
            flat.tofile(f); scans.tofile(f)
            np.stack([pose[:, 3], pose[:, 6], pose[:, 7], pose[:, 8], pose[:, 12], ctrl[:, 0], ctrl[:, 1]], axis=1).tofile(f)
        r = subprocess.run([harness, str(src), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, dtype=np.float64).reshape(n_cars, 2)
        want = nm.evaluate(net, scans, pose, ctrl)
        np.testing.assert_array_equal(got, want, err_msg=f"{case}, slot {s}")
        assert (np.abs(want).max() > 0) == (s != 3), (case, s)


def no_load():
    raise AssertionError("the library was loaded before the arguments were checked")


def small_spec(**over):
    from ft_grandprix_amd.net import NetSpec
    net = nm.random_net(np.random.default_rng(1), (17, 8, 2), pool=4, max_range=3.0, beam_first=2, use_state=True)
    return NetSpec(net["layers"], **{**{k: v for k, v in net.items() if k != "layers"}, **over})


@pytest.mark.parametrize("nets", [{4: "spec"}, {-1: "spec"}, {"net7": "spec"}, {0: "spec_outside"}, {0: "spec_pool"}, {0: 3.0}, ["spec"]])
def test_device_vec_env_checks_the_networks_before_a_handle_exists(nets, monkeypatch):
    from ft_grandprix_amd import capi, vec
    specs = {"spec": small_spec(), "spec_outside": small_spec(beam_first=1), "spec_pool": small_spec(pool=3, beam_first=3)}
    nets = {k: specs.get(v, v) for k, v in nets.items()} if isinstance(nets, dict) else nets
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises((ValueError, TypeError)):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, cars_per_env=2, roster=["agent", "net0"], nets=nets)


def test_device_vec_env_accepts_a_valid_network_up_to_the_load(monkeypatch):
    from ft_grandprix_amd import capi, vec

    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(capi, "load", reached)
    with pytest.raises(Reached):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, cars_per_env=2, roster=["agent", "net0"], nets={0: small_spec()})
    with pytest.raises(ValueError):
        vec.DeviceVecEnv("small-circle", n_envs=4, n_rays=64, cars_per_env=2, roster=["agent", "net4"])


@pytest.mark.parametrize("change", [dict(max_range=0.0), dict(max_range=float("inf")), dict(pool=0), dict(n_beams=0), dict(n_beams=300),
                                    dict(hidden_act="gelu"), dict(out_act="sigmoid"), dict(out_scale=(1.0, float("nan"))),
                                    dict(out_offset=(float("inf"), 0.0)), dict(out_scale=(1.0,))])
def test_net_spec_refuses_bad_fields(change, monkeypatch):
    from ft_grandprix_amd import capi
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        small_spec(**change)


def test_net_spec_refuses_bad_layers(monkeypatch):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.net import NetSpec
    monkeypatch.setattr(capi, "load", no_load)
    z = lambda *s: np.zeros(s, dtype=np.float32)                    # noqa: E731
    kw = dict(pool=4, max_range=3.0, beam_first=2, n_beams=12)
    for layers in ([(z(3, 12), z(3))], [(z(2, 11), z(2))], [(z(129, 12), z(129)), (z(2, 129), z(2))], [(z(2, 12), z(3))], [],
                   [(z(4, 12), z(4))] * 4 + [(z(2, 4), z(2))]):
        with pytest.raises(ValueError):
            NetSpec(layers, **kw)


def test_from_torch_and_the_npz_round_trip(tmp_path, monkeypatch):
    import torch
    from ft_grandprix_amd import capi, net
    monkeypatch.setattr(capi, "load", no_load)
    torch.manual_seed(0)
    module = torch.nn.Sequential(torch.nn.Linear(17, 8), torch.nn.Tanh(), torch.nn.Linear(8, 2), torch.nn.Tanh())
    spec = net.from_torch(module, pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True, out_scale=(3.0, 0.5), out_offset=(3.0, 0.0))
    assert (spec.hidden_act, spec.out_act, spec.widths) == ("tanh", "tanh", (17, 8, 2))
    assert spec.layers[0][0].shape == (8, 17) and spec.layers[1][0].shape == (2, 8)           # [out][in]
    np.testing.assert_array_equal(spec.layers[0][0], module[0].weight.detach().numpy())
    flat = spec.flat_params()
    assert flat.dtype == np.float32 and flat.size == 8 * 17 + 8 + 2 * 8 + 2
    np.testing.assert_array_equal(flat[:8 * 17].reshape(8, 17), spec.layers[0][0])
    np.testing.assert_array_equal(flat[8 * 17:8 * 17 + 8], spec.layers[0][1])
    spec.save(tmp_path / "driver.npz")
    back = net.load(tmp_path / "driver.npz")
    assert back.input_fields() == spec.input_fields() and back.shape_key() == spec.shape_key()
    np.testing.assert_array_equal(back.flat_params(), flat)
    # the model runs what torch runs, up to TANH and the order of the sums
    x = np.random.default_rng(2).uniform(0, 1, (6, 17)).astype(np.float32)
    want = module(torch.from_numpy(x)).detach().numpy()
    got = nm.forward(x, spec.layers, spec.hidden_act, spec.out_act)
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-6)
    relu = net.from_torch(torch.nn.Sequential(torch.nn.Linear(12, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2)), pool=4, max_range=3.0, beam_first=2, n_beams=12)
    assert (relu.hidden_act, relu.out_act) == ("relu", "identity")
    for bad in (torch.nn.Linear(12, 2), torch.nn.Sequential(torch.nn.Linear(12, 2), torch.nn.Sigmoid()),
                torch.nn.Sequential(torch.nn.Conv1d(1, 1, 3)), torch.nn.Sequential(torch.nn.Tanh(), torch.nn.Linear(12, 2)),
                torch.nn.Sequential(torch.nn.Linear(12, 4), torch.nn.ReLU(), torch.nn.Linear(4, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2))):
        with pytest.raises((TypeError, ValueError)):
            net.from_torch(bad, pool=4, max_range=3.0, beam_first=2, n_beams=12)


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_policy_eval_equals_the_model_on_every_shape():
    """The four slots with different random networks on scans holding -1, 0, M and values above M: one layer 12 -> 2 at 64 rays;
    85 -> 64 -> 64 -> 2 tanh with state at 1080 rays; 85 -> 37 -> 2 relu; the limits 256 -> 128 -> 128 -> 128 -> 2 at 1344 rays; pool 1.
    An infinite weight and a finished car give (0, 0)."""
    assert "policy_eval ok" in run_child("policy_eval")


@pytest.mark.gpu
def test_closed_loop_in_one_launch_equals_the_oracle_driven_by_the_model():
    """19 envs on small-circle, rollout("net0", 50) three times; the oracle twin is driven per step through the host by the model."""
    assert "closed loop ok" in run_child("closed_loop")


@pytest.mark.gpu
def test_roster_with_network_slots_equals_a_twin_stepped_through_the_host():
    assert "roster ok" in run_child("roster")


@pytest.mark.gpu
def test_device_step_net_slot_sees_what_an_agent_is_given():
    """roster ["agent", "net0"] against ["agent", "agent"] whose second agent is the model on the obs and state of the call before,
    over 40 calls with auto-resets: the train -> deploy contract."""
    assert "device step ok" in run_child("device_step")


@pytest.mark.gpu
def test_multitrack_with_the_dynamics_table_on():
    assert "multitrack ok" in run_child("multitrack")


@pytest.mark.gpu
def test_device_setter_replaces_the_parameters_in_stream_order():
    assert "device setter ok" in run_child("device_setter")


@pytest.mark.gpu
def test_launches_without_a_network_run_the_kernels_they_ran():
    assert "no network ok" in run_child("no_network")


@pytest.mark.gpu
def test_errors_leave_a_defined_slot_in_force():
    assert "errors ok" in run_child("errors")
