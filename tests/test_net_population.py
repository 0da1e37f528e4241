"""Network populations (include/ftgp.h "Network populations": ftgp_set_net_population / ftgp_set_net_population_device /
ftgp_get_net_population; ft_grandprix_amd/net.py: param_count, with_params, stack_params; ft_grandprix_amd/vec.py:
DeviceVecEnv.set_population / population).

CPU: the binding; the argument checks, which run before the library is loaded; the NetSpec round trips; the member-strided layout
conversion the library ships (csrc/ftgp_net.h, compiled for the host by tools/net_layout_check.cpp, also under the address and
undefined-behaviour sanitizers) against numpy.

GPU: every scenario runs in a fresh child process (tests/net_population_child.py) that imports torch before libftgp.so is loaded, one
at a time, each under a time limit (tests/children.py).  The criterion throughout is equality to the bit, no tolerance: env e of a
handle with a population leaves what env e of a twin leaves whose slot holds member env_member[e]'s parameters through plain
ftgp_set_net -- M members, M twin runs, each compared on its own envs -- in lidar, pose, progress, ctrl and steps.  The plain path is
held to the numpy model by tests/test_net_driver.py.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "net_population_child.py")
ENTRIES = ("set_net_population", "set_net_population_device", "get_net_population")

run_child = functools.partial(children.run_child, CHILD, timeout=300)


def no_load():
    raise AssertionError("the library was loaded before the arguments were checked")


def small_spec(seed=0, hidden=8, **over):
    from ft_grandprix_amd.net import NetSpec
    rng = np.random.default_rng(seed)
    layers = [(rng.standard_normal((hidden, 17)).astype(np.float32), rng.standard_normal(hidden).astype(np.float32)),
              (rng.standard_normal((2, hidden)).astype(np.float32), rng.standard_normal(2).astype(np.float32))]
    return NetSpec(layers, **{**dict(pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True), **over})


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_binding_declares_the_population_entries():
    from ft_grandprix_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for name in ENTRIES:
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None, name
        assert f"int ftgp_{name}(FtgpEnv *env" in header, name
    assert len(lib.fn("set_net_population").argtypes) == 5 and len(lib.fn("set_net_population_device").argtypes) == 5
    assert len(lib.fn("get_net_population").argtypes) == 6
    for method in ENTRIES:
        assert callable(getattr(capi.Env, method))
    assert "#define FTGP_ABI_VERSION 5" in header                      # the change only adds entries
    assert "taken as member 0" in header                                # the device setter's rule for a map entry out of range


def test_population_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    from ft_grandprix_amd import capi
    monkeypatch.setattr(capi, "load", no_load)
    ok = np.zeros((3, 10), dtype=np.float32)
    p, m = capi.net_population_args(ok, [2, 0, 0, 1, 2, 1, 0], 7, count=10)
    assert p.shape == (3, 10) and m.dtype == np.int32 and m.tolist() == [2, 0, 0, 1, 2, 1, 0]
    assert capi.net_population_args(ok, None, 7)[1] is None and capi.net_population_args(None, None, 7) == (None, None)
    for params, env_member, count in ((ok.astype(np.float64), None, None),              # dtype
                                      (ok[0], None, None), (ok[None], None, None),        # not [n_members, count]
                                      (np.zeros((0, 10), dtype=np.float32), None, None),  # no member
                                      (np.zeros((8, 10), dtype=np.float32), None, None),  # more members than envs
                                      (ok, None, 11),                                     # another count
                                      (ok, [0, 1, 2, 3, 0, 1, 2], None), (ok, [0, 1, 2, -1, 0, 1, 2], None),     # map range
                                      (ok, [0, 1, 2], None), (ok, np.zeros((7, 1), dtype=np.int32), None),        # map shape
                                      (ok, np.zeros(7, dtype=np.float32), None), (ok, np.zeros(7, dtype=bool), None),
                                      (None, [0] * 7, None)):
        with pytest.raises(ValueError):
            capi.net_population_args(params, env_member, 7, count)


def test_stack_params_and_with_params_round_trip(monkeypatch):
    from ft_grandprix_amd import capi, net
    monkeypatch.setattr(capi, "load", no_load)
    specs = [small_spec(s) for s in range(3)]
    assert specs[0].param_count == 8 * 17 + 8 + 2 * 8 + 2 == specs[0].flat_params().size
    rows = net.stack_params(specs)
    assert rows.dtype == np.float32 and rows.shape == (3, specs[0].param_count)
    for k, s in enumerate(specs):
        np.testing.assert_array_equal(rows[k], s.flat_params())
        back = specs[0].with_params(rows[k])
        assert back.shape_key() == s.shape_key() and back is not specs[0]
        np.testing.assert_array_equal(back.flat_params(), rows[k])
        for (W, b), (W0, b0) in zip(back.layers, s.layers):
            np.testing.assert_array_equal(W, W0); np.testing.assert_array_equal(b, b0)
    np.testing.assert_array_equal(specs[0].flat_params(), rows[0])     # with_params left the spec it was asked of alone
    import torch
    np.testing.assert_array_equal(specs[0].with_params(torch.from_numpy(rows[2])).flat_params(), rows[2])
    for bad in (rows[0][:-1], rows[0].astype(np.float64), rows):
        with pytest.raises(ValueError):
            specs[0].with_params(bad)


def test_stack_params_refuses_specs_of_another_shape(monkeypatch):
    from ft_grandprix_amd import capi, net
    monkeypatch.setattr(capi, "load", no_load)
    a = small_spec(0)
    for other in (small_spec(1, hidden=9), small_spec(1, max_range=4.0), small_spec(1, out_scale=(2.0, 1.0)), small_spec(1, hidden_act="relu")):
        with pytest.raises(ValueError):
            net.stack_params([a, other])
    for bad in ([], [a, a.flat_params()]):
        with pytest.raises(ValueError):
            net.stack_params(bad)


def test_device_vec_env_checks_a_population_before_a_handle_exists(monkeypatch):
    from ft_grandprix_amd import capi, vec
    monkeypatch.setattr(capi, "load", no_load)
    for method in ("set_population", "population"):
        assert callable(getattr(vec.DeviceVecEnv, method))
    env = vec.DeviceVecEnv.__new__(vec.DeviceVecEnv)                   # the checks in front of the library calls, on an object without a handle
    env.n_envs, env._nets, env._pops, env.env = 7, {0: (small_spec().shape_key(), None)}, {}, None
    rows = np.zeros((3, small_spec().param_count), dtype=np.float32)
    for slot, params, env_member in ((1, rows, None), (4, rows, None), (0, rows.astype(np.float64), None), (0, rows[0], None),
                                     (0, rows, [0, 1, 2, 3, 0, 1, 2]), (0, np.zeros((8, rows.shape[1]), dtype=np.float32), None), (0, rows[:, :-1], None), (0, None, [0] * 7),
                                     (0, rows, "keep"), (0, rows, "same")):          # ("keep" needs a population of as many members)
        with pytest.raises(ValueError):
            env.set_population(slot, params, env_member)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def layout_harness(tmp_path_factory, request):
    """tools/net_layout_check.cpp built by the host compiler, plain and with the address and undefined-behaviour sanitizers (a
    stand-alone program: nothing of it is loaded into python)."""
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    from tests.test_collect import sanitizers_available
    tmp = tmp_path_factory.mktemp("layout")
    out = str(tmp / f"net_layout_check_{request.param}")
    flags = ["-O2", "-std=c++17"]
    if request.param == "sanitized":
        # (the runtimes linked statically where the compiler knows the switches: the program then needs nothing of its environment)
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]          # (clang links them statically anyway)
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static]
        if not sanitizers_available(cxx, flags, tmp):       # decided on an empty program, before the code under test is touched
            pytest.skip("the host compiler has no sanitizer runtimes (an empty program does not build and run with them)")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "net_layout_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.mark.parametrize("widths, n_members", [((17, 16, 2), 3), ((17, 100, 2), 2), ((85, 64, 64, 2), 5), ((256, 128, 128, 128, 2), 2), ((12, 2), 4), ((3, 65, 1, 2), 1)])
def test_member_strided_layout_conversion_equals_numpy(layout_harness, tmp_path, widths, n_members):
    """The shipped conversion (csrc/ftgp_net.h: what the setters, the getters and ftgp_net_params_kernel call) against numpy: per member
    and layer Wt[n_in][ld] = W transposed with ld = n_out rounded up to 64, then b[ld], zeros in the padding, members a stride apart
    that is the set's size rounded up to 64 floats; the way back returns every float."""
    rng = np.random.default_rng(len(widths) * 1000 + n_members)
    n_layers = len(widths) - 1
    count = sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(n_layers))
    src = rng.standard_normal((n_members, count)).astype(np.float32)
    src[src == 0] = 1.0                                                  # (a zero could not be told from the padding)
    head = np.zeros(7, dtype=np.int32)
    head[0], head[1:1 + len(widths)], head[6] = n_layers, widths, n_members
    (tmp_path / "in.bin").write_bytes(head.tobytes() + src.tobytes())
    r = subprocess.run([layout_harness, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    got_count, lib, stride = np.frombuffer(raw, dtype=np.int32, count=3)
    want_lib = sum((widths[l] + 1) * 64 * -(-widths[l + 1] // 64) for l in range(n_layers))
    assert (got_count, lib, stride) == (count, want_lib, -(-want_lib // 64) * 64) and stride % 64 == 0
    img = np.frombuffer(raw, dtype=np.float32, count=n_members * stride, offset=12).reshape(n_members, stride)
    back = np.frombuffer(raw, dtype=np.float32, count=n_members * count, offset=12 + 4 * n_members * stride).reshape(n_members, count)
    index = np.frombuffer(raw, dtype=np.int32, count=count + 2, offset=12 + 4 * n_members * (stride + count))
    want = np.zeros((n_members, stride), dtype=np.float32)
    for m in range(n_members):
        o = p = 0
        for l in range(n_layers):
            n_in, n_out = widths[l], widths[l + 1]
            ld = -(-n_out // 64) * 64
            W = src[m, p:p + n_out * n_in].reshape(n_out, n_in); p += n_out * n_in
            b = src[m, p:p + n_out]; p += n_out
            Wt = np.zeros((n_in, ld), dtype=np.float32); Wt[:, :n_out] = W.T
            want[m, o:o + n_in * ld] = Wt.ravel(); o += n_in * ld
            want[m, o:o + n_out] = b; o += ld
    np.testing.assert_array_equal(img.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(back.view(np.uint32), src.view(np.uint32))
    assert (img != 0).sum() == n_members * count, "the padding is zeros and nothing else"
    assert index[count] == -1 and index[count + 1] == -1
    assert len(set(index[:count].tolist())) == count and index[:count].min() >= 0 and index[:count].max() < lib
    np.testing.assert_array_equal(want[0][index[:count]], src[0])


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_rollout_with_a_population_equals_the_members_twins():
    """3 members on 7 envs of small-circle with the map [2, 0, 0, 1, 2, 1, 0] and with NULL (e % 3), rollout("net0", 40)."""
    assert "rollout ok" in run_child("rollout")


@pytest.mark.gpu
def test_rollout_with_cars_of_different_members_in_one_workgroup():
    """The same with FTGP_CARS_PER_BLOCK=4 set before the library loads: workgroups of four envs hold members 2, 0, 0, 1 and 2, 1, 0."""
    out = run_child("rollout", cpb=4)
    assert "rollout ok" in out
    assert "ftgp_create: 4 cars x" in out, "the switch was not honoured: no workgroup held cars of different members"


@pytest.mark.gpu
def test_shapes_that_take_the_other_code_paths():
    """A hidden layer of 100 neurons (the WIDE rows, ld = 128; 2002 parameters, no multiple of 64) and 85 inputs at 512 rays (the second
    input register) with two hidden layers, in slot 2."""
    assert "shapes ok" in run_child("shapes")


@pytest.mark.gpu
def test_multi_car_roster_with_a_population_on_one_slot():
    """cars_per_env = 4, roster net0, net1, fast, nidc; net0 has rival inputs (n_rivals = 2) and a population, net1 has none; one track
    and a multi-track handle (small-circle, circle)."""
    assert "roster ok" in run_child("roster")


@pytest.mark.gpu
def test_device_setter_replaces_members_and_map_in_stream_order():
    """Parameters and map replaced between two launches from torch tensors on a stream of their own equal the host setter's; every
    member comes back to the bit; a map entry out of range is member 0; the same tensors twice and all-zero members evaluate as the
    host setter's; the device setter's refusals; 1100 members, more than the conversion kernel's grid has rows."""
    assert "device setter ok" in run_child("device_setter")


@pytest.mark.gpu
def test_policy_eval_takes_the_member_of_the_cars_env():
    assert "policy_eval ok" in run_child("policy_eval")


@pytest.mark.gpu
def test_collect_on_a_population_slot_equals_the_members_twins():
    """DeviceVecEnv.collect(8, slot=0, next_inputs=True) with a fixed noise tensor, auto-reset and max_episode_steps = 6: inputs, mean,
    action, reward, the ends and next_inputs per env equal its member's twin; set_population the host way and the device way."""
    assert "collect ok" in run_child("collect")


@pytest.mark.gpu
def test_an_env_that_loads_another_envs_state_keeps_its_own_member():
    assert "env states ok" in run_child("env_states")


@pytest.mark.gpu
def test_removal_restores_the_single_set():
    """n_members = 0 and ftgp_set_net both leave a handle that rolls out as one that never had a population; ftgp_reset keeps one; a
    launch that names no network runs the kernel it ran."""
    assert "removal ok" in run_child("removal")


@pytest.mark.gpu
def test_refusals_leave_the_slot_as_it_was():
    """Every FTGP_ERR_ARG and FTGP_ERR_STATE case of the three entries, on a slot without and with a population: the slot evaluates as
    before each."""
    assert "errors ok" in run_child("errors")
