"""Network drivers with rival inputs (include/ftgp.h: ftgp_set_net_rivals / ftgp_get_net_rivals; net.NetSpec(rivals=, n_rivals=);
DeviceVecEnv follows the spec).

CPU: the struct and the binding; NetSpec's checks, which run before the library is loaded, and its behaviour; the shipped element
operations (csrc/ftgp_rival.h, csrc/ftgp_frame.h and csrc/ftgp_net.h, compiled for the host by tools/net_check.cpp --rivals, also under
the address and undefined-behaviour sanitizers) against the model of the header's text (tests/net_rivals_model.py = net_frame_model +
rival_model), bit for bit, on envs that reach every branch of the rival row.

GPU: every scenario in a fresh child process (tests/net_rivals_child.py), equality to the bit with the model throughout.
"""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import children
from tests import frame_model as fm
from tests import net_model as nm
from tests import net_rivals_model as nrm
from tests import rival_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "net_rivals_child.py")
run_child = functools.partial(children.run_child, CHILD, timeout=300)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_struct_and_binding():
    from ft_grandprix_amd import capi
    assert ctypes.sizeof(capi.FtgpNetRivals) == 16
    assert [(n, getattr(capi.FtgpNetRivals, n).offset) for n, _ in capi.FtgpNetRivals._fields_] == [("enabled", 0), ("n_rivals", 4), ("reserved", 8)]
    assert ctypes.sizeof(capi.FtgpNetDesc) == 68 and ctypes.sizeof(capi.FtgpNetFrame) == 16          # unchanged
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for name in ("set_net_rivals", "get_net_rivals"):
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None, name
        assert f"int ftgp_{name}(FtgpEnv *env, int slot, " in header, name
    assert len(lib.fn("set_net_rivals").argtypes) == 6 and len(lib.fn("get_net_rivals").argtypes) == 3
    assert "typedef struct FtgpNetRivals {" in header and "Rival rows as inputs are not part of this" not in header
    for method in ("set_net", "net", "net_frame", "net_rivals", "get_net"):
        assert callable(getattr(capi.Env, method))
    # the handle-free checks: net_desc's return shape is what it was
    net = nrm.random_net(np.random.default_rng(1), (8,), n_beams=12, lookahead=3, lookahead_stride=2, n_rivals=3, pool=4, max_range=3.0, beam_first=2)
    out = capi.net_desc(net["layers"], **nrm.fields(net))
    assert len(out) == 2 and isinstance(out[0], capi.FtgpNetDesc) and out[1].size == 8 * (27 + 28) + 8 + 2 * 8 + 2
    r = capi.net_rivals(False, 3)
    assert (r.enabled, r.n_rivals, tuple(r.reserved)) == (1, 3, (0, 0))
    r = capi.net_rivals(True)
    assert (r.enabled, r.n_rivals) == (1, 0) and capi.net_rival_inputs(r) == 4 and capi.net_rival_inputs(capi.net_rivals()) == 0


def no_load():
    raise AssertionError("the library was loaded before the arguments were checked")


def small_spec(n_beams=12, hidden=(8,), **rivals):
    from ft_grandprix_amd.net import NetSpec
    n = rivals.get("n_rivals", 0)
    n = n if isinstance(n, int) and n > 0 else 0                    # (a refused value: any width will do, the fields are checked first)
    width0 = n_beams + 5 + ((4 + 8 * n) if (rivals.get("rivals") or n > 0) else 0)
    net = nm.random_net(np.random.default_rng(1), (width0, *hidden, 2), pool=4, max_range=3.0, beam_first=2, use_state=True)
    net["n_beams"] = n_beams
    return NetSpec(net["layers"], **{**nrm.fields(net), **rivals})


@pytest.mark.parametrize("rivals", [dict(n_rivals=8), dict(n_rivals=-1), dict(rivals=True, n_rivals=1.5), dict(rivals=False, n_rivals=8)])
def test_net_spec_refuses_bad_rival_fields(rivals, monkeypatch):
    from ft_grandprix_amd import capi
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        small_spec(**rivals)


def test_net_spec_refuses_257_inputs_reached_through_the_rival_block(monkeypatch):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.net import NetSpec
    monkeypatch.setattr(capi, "load", no_load)
    z = lambda *s: np.zeros(s, dtype=np.float32)                    # noqa: E731
    kw = dict(pool=4, max_range=8.0, beam_first=42, use_state=True)
    NetSpec([(z(2, 256), z(2))], n_beams=155, lookahead=16, n_rivals=7, **kw)       # 155 + 5 + 36 + 60 = 256: the limit
    with pytest.raises(ValueError, match="257"):
        NetSpec([(z(2, 257), z(2))], n_beams=156, lookahead=16, n_rivals=7, **kw)
    NetSpec([(z(2, 197), z(2))], n_beams=156, lookahead=16, **kw)                   # the same beams without the rival block are fine
    with pytest.raises(ValueError):
        NetSpec([(z(2, 197), z(2))], n_beams=156, lookahead=16, n_rivals=1, **kw)   # the first layer must be as wide as the true n_in


def test_net_spec_with_rival_inputs(tmp_path, monkeypatch):
    from ft_grandprix_amd import capi, net
    monkeypatch.setattr(capi, "load", no_load)
    spec = small_spec(n_rivals=3)
    assert spec.rivals is True and spec.n_rivals == 3 and spec.n_rival == 28 and spec.n_frame == 0
    assert spec.n_in == 12 + 5 + 4 + 24 and spec.widths == (45, 8, 2) and spec.widths[0] == spec.n_in
    assert spec.flat_params().size == 8 * 45 + 8 + 2 * 8 + 2
    fields = spec.input_fields()
    assert (fields["rivals"], fields["n_rivals"]) == (True, 3)
    only_fixed = small_spec(rivals=True)
    assert only_fixed.n_in == 12 + 5 + 4 and only_fixed.n_rivals == 0 and only_fixed.n_rival == 4
    assert small_spec().n_in == 17 and small_spec().rivals is False and small_spec().n_rival == 0
    # two specs that differ only in n_rivals cannot replace one another through the device setter
    other = small_spec(n_rivals=2)
    assert other.shape_key() != spec.shape_key() and small_spec(n_rivals=3).shape_key() == spec.shape_key()
    # ... not even where the widths agree: 4 + 8 * 2 rival entries against 4 + 2 * 8 frame entries
    from ft_grandprix_amd.net import NetSpec
    z = lambda *s: np.zeros(s, dtype=np.float32)                    # noqa: E731
    kw = dict(pool=4, max_range=3.0, beam_first=2, n_beams=12)
    p, q = NetSpec([(z(2, 32), z(2))], n_rivals=2, **kw), NetSpec([(z(2, 32), z(2))], lookahead=8, **kw)
    assert p.widths == q.widths and p.shape_key() != q.shape_key()
    # the npz round trip
    both = NetSpec([(z(2, 12 + 10 + 28), z(2))], lookahead=3, lookahead_stride=2, n_rivals=3, **kw)
    both.save(tmp_path / "rivals.npz")
    back = net.load(tmp_path / "rivals.npz")
    assert back.input_fields() == both.input_fields() and back.shape_key() == both.shape_key()
    assert (back.rivals, back.n_rivals, back.frame, back.lookahead, back.lookahead_stride) == (True, 3, True, 3, 2)
    np.testing.assert_array_equal(back.flat_params(), both.flat_params())
    # a file written before the rival inputs existed: neither of the two keys, rivals are off
    plain = small_spec()
    plain.save(tmp_path / "new.npz")
    with np.load(tmp_path / "new.npz") as f:
        old = {k: f[k] for k in f.files if k not in ("rivals", "n_rivals")}
    assert len(old) == len(np.load(tmp_path / "new.npz").files) - 2
    np.savez(tmp_path / "old.npz", **old)
    back = net.load(tmp_path / "old.npz")
    assert back.rivals is False and back.n_rivals == 0 and back.shape_key() == plain.shape_key()
    # from_torch
    import torch
    module = torch.nn.Sequential(torch.nn.Linear(12 + 5 + 12 + 20, 8), torch.nn.Tanh(), torch.nn.Linear(8, 2), torch.nn.Tanh())
    t = net.from_torch(module, pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True, lookahead=4, n_rivals=2)
    assert t.widths == (49, 8, 2) and (t.rivals, t.n_rivals, t.lookahead) == (True, 2, 4)
    with pytest.raises(ValueError):
        net.from_torch(module, pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True, lookahead=4, n_rivals=3)


def sanitizers_available(cxx, flags, tmp):
    src = tmp / "empty.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp / "empty")
    if subprocess.run([cxx, *flags, str(src), "-o", exe], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True, text=True).returncode == 0


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("net_rivals")
    out = str(tmp / f"net_check_{request.param}")
    flags = ["-O2", "-ffp-contract=off", "-std=c++17"]
    if request.param == "sanitized":
        # a stand-alone program with the runtimes linked in (statically where the compiler knows the switches): it needs nothing of its environment
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static]
        if not sanitizers_available(cxx, flags, tmp):
            pytest.skip("the host compiler has no sanitizer runtimes (an empty program does not build and run with them)")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "net_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_harness(harness, tmp_path, name, net, n_rays, scans, pose, ctrl, path, race):
    """(inputs float32 [n, n_in], controls float64 [n, 2]) of tools/net_check --rivals."""
    n_cars, flat = len(pose), nrm.flat_params(net)
    widths = [W.shape[0] for W, _ in net["layers"]] + [0] * (4 - len(net["layers"]))
    src, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([n_rays, n_cars, net["pool"], net["beam_first"], net["n_beams"], int(net["use_state"]), len(net["layers"]), *widths,
                  nm.ACT[net["hidden_act"]], nm.ACT[net["out_act"]], flat.size], dtype=np.int32).tofile(f)
        np.array([net["max_range"], *net["out_scale"], *net["out_offset"]], dtype=np.float32).tofile(f)
        np.array([int(net["frame"]), net["lookahead"], net["lookahead_stride"]], dtype=np.int32).tofile(f)
        np.array([int(net["rivals"]), net["n_rivals"], race["cpe"]], dtype=np.int32).tofile(f)
        flat.tofile(f); np.ascontiguousarray(scans, dtype=np.float32).tofile(f)
        np.stack([pose[:, 3], pose[:, 6], pose[:, 7], pose[:, 8], pose[:, 12], ctrl[:, 0], ctrl[:, 1], pose[:, 0], pose[:, 1]], axis=1).tofile(f)
        np.ascontiguousarray(path, dtype=np.float64).tofile(f)
        np.asarray(race["abs_completion"], dtype=np.int32).tofile(f); np.asarray(race["finished"], dtype=np.int32).tofile(f)
        np.asarray(race["finish_step"], dtype=np.int64).tofile(f)
    r = subprocess.run([harness, "--rivals", str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w = nrm.n_in(net)
    assert r.stdout.count("inputs") == n_cars and r.stdout.count("speed") == n_cars
    raw = open(out, "rb").read()
    assert len(raw) == 4 * n_cars * w + 16 * n_cars
    return np.frombuffer(raw[:4 * n_cars * w], dtype=np.float32).reshape(n_cars, w), np.frombuffer(raw[4 * n_cars * w:], dtype=np.float64).reshape(n_cars, 2)


def test_the_scene_list_reaches_the_situations_it_names():
    """By the model of the header's text and by rival_model.independent_rows."""
    path = fm.square_path()
    scenes = nrm.all_scenes()

    def look(name):
        pose, race = nrm.scene_env(scenes[name])
        args = (path, pose, race["abs_completion"], race["finished"], race["finish_step"], race["cpe"], 7)
        rows, g, place, mates = rm.rival_rows64(*args)
        irows, iplace, imates = rm.independent_rows(*args)
        np.testing.assert_array_equal(place, iplace, err_msg=name)
        np.testing.assert_array_equal(mates, imates, err_msg=name)
        np.testing.assert_allclose(rows, irows, rtol=0, atol=1e-12, err_msg=name)
        _, s, c, off = rm.progress64(path, pose, race["abs_completion"])
        return rows, g, place, mates, s, c, off
    rows, g, place, mates, *_ = look("left, looking west, equal g")
    assert g[0] == g[1] and list(place) == [1, 2]                                        # equal g: the smaller slot is ahead
    rows, g, place, mates, *_ = look("equal d2")
    d2 = rows[1, 4 + rm.FWD] ** 2 + rows[1, 4 + rm.LEFT] ** 2, rows[1, 12 + rm.FWD] ** 2 + rows[1, 12 + rm.LEFT] ** 2
    assert d2[0] == d2[1] and list(mates[1, :3]) == [0, 2, -1]                           # equal d2: the smaller slot first
    rows, g, place, mates, *_ = look("one spot")
    assert rows[0, 4 + rm.FWD] == 0.0 and rows[0, 4 + rm.LEFT] == 0.0 and rows[0, 4 + rm.PRESENT] == 1.0 and list(place) == [1, 2]
    rows, g, place, mates, s, c, off = look("half a lap apart")
    assert s[1] - s[0] == 50.0 and rows[0, 4 + rm.TRACK_GAP] == -50.0 and rows[1, 4 + rm.TRACK_GAP] == -50.0      # +50 wraps, -50 stays
    rows, g, place, mates, s, c, off = look("track_gap +50 and -50")
    assert s[1] - s[0] == 50.0 and rows[0, 4 + rm.TRACK_GAP] == -50.0 and rows[1, 4 + rm.TRACK_GAP] == -50.0
    rows, g, place, mates, s, c, off = look("f wraps: c = 0, s = 99.5")
    assert c[0] == 0 and s[0] == 99.5 and g[0] == 99.5 and g[1] == 100.5 and list(place) == [2, 1, 3]           # f = 99.5 - 100
    rows, g, place, mates, s, c, off = look("across the line")
    assert c[0] == 0 and s[0] == 99.5 and rows[0, 4 + rm.TRACK_GAP] == s[1] - 99.5 + 100.0
    rows, g, place, mates, s, c, off = look("off-track mate")
    assert off[1] and not off[0] and g[1] == 6.0 and g[0] == 6.5 and rows[0, 4 + rm.PRESENT] == 1.0             # f_b = 0 off the track, still a mate
    rows, g, place, mates, *_ = look("finishers")
    assert list(place) == [4, 2, 5, 3, 1] and list(mates[0, :2]) == [2, -1] and (mates[[1, 3, 4]] == -1).all()      # equal finish_step: the slot decides
    assert rows[1, rm.N_RACING] == 2 and (rows[1, 2:] == 0).all()                                                # a finished a: its place, no gaps, no mates
    rows, g, place, mates, *_ = look("finishers, different steps")
    assert list(place) == [3, 2, 1, 4] and list(mates[0, :2]) == [3, -1]
    rows, g, place, mates, *_ = look("finishers, steps past 2^32")
    assert list(place) == [2, 1, 3]                                                                              # 2^32 + 5 > 7: the 64-bit order
    rows, g, place, mates, *_ = look("everyone finished")
    assert list(place) == [1, 2] and (rows[:, 1:] == 0).all()
    rows, g, place, mates, *_ = look("alone")
    assert list(rows[0]) == [1, 1, 0, 0] + [0] * 56


HOST_SHAPES = [dict(n_rivals=0), dict(n_rivals=1), dict(n_rivals=3, lookahead=2, lookahead_stride=3), dict(n_rivals=7), dict(n_rivals=7, use_state=False),
               dict(n_rivals=3, use_state=False, frame=True), dict(rivals=False)]


def host_case(harness, tmp_path, name, path, cars, rng, shape):
    pose, race = nrm.scene_env(cars)
    pose[:, 12] = rng.uniform(-2, 2, len(pose))
    n_rays = 64
    base = dict(pool=4, max_range=3.0, beam_first=2, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
    net = nrm.random_net(rng, (9,), n_beams=12, **{**base, **shape})
    ctrl = np.stack([rng.uniform(0, 7, len(pose)), rng.uniform(-1, 1, len(pose))], axis=1)
    scans = nm.eval_scans(rng, len(pose), n_rays, net["max_range"])
    got_x, got_u = run_harness(harness, tmp_path, name, net, n_rays, scans, pose, ctrl, path, race)
    want_u, want_x = nrm.evaluate(net, scans, pose, ctrl, path, race, finished=race["finished"] != 0)
    np.testing.assert_array_equal(got_x.view(np.int32), want_x.view(np.int32), err_msg=f"{name}, {shape}: inputs")
    np.testing.assert_array_equal(got_u, want_u, err_msg=f"{name}, {shape}: controls")
    return want_x, race


def test_host_harness_equals_the_model_on_the_hand_scenes(harness, tmp_path):
    path = fm.square_path()
    rng = np.random.default_rng(31)
    for k, (name, cars) in enumerate(nrm.all_scenes().items()):
        for j, shape in enumerate(HOST_SHAPES):
            host_case(harness, tmp_path, f"scene{k}_{j}", path, cars, rng, shape)


@pytest.mark.parametrize("cpe", [1, 2, 3, 5, 8])
def test_host_harness_equals_the_model_on_random_envs(harness, tmp_path, cpe):
    rng = np.random.default_rng(100 + cpe)
    more = fewer = 0
    for which, path in (("square", fm.square_path()), ("skew", fm.skew_path())):
        for r in range(3):
            cars = nrm.random_env(path, rng, cpe, finished=(0, 1, 2)[r] if cpe > 2 else 0)
            for j, shape in enumerate(HOST_SHAPES):
                x, race = host_case(harness, tmp_path, f"{which}{r}_{j}", path, cars, rng, shape)
                n = shape.get("n_rivals", 0)
                racing = int((race["finished"] == 0).sum())
                more += int(n > racing - 1); fewer += int(0 < n < racing - 1)
    assert more > 0 and (fewer > 0 or cpe < 3)                      # more slots than mates, and fewer


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_policy_eval_equals_the_model_and_the_inputs_end_with_the_rival_rows():
    """set_pose puts the hand scenes and random envs of 1, 2, 3, 5 and 8 cars on the open-field square (8 rays, one identity layer),
    finishers by teleport on `track` and by lap_target 0: ftgp_policy_eval(NETk) equals the model, the act kernel's recorded inputs equal
    the model's and end with ftgp_get_rivals(n_rivals).  Shapes on small-circle: a rival block that begins at lane 63, one across lanes
    127 / 128, n_in = 256 with n_rivals 7 and lookahead 16 at 1344 rays, n_rivals 0, no state and no frame inputs, one car per env."""
    assert "policy_eval ok" in run_child("policy_eval")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["5x3", "3x8"])
def test_closed_loop_in_one_launch_equals_the_twin_driven_by_the_model(shape):
    """5 envs x 3 cars and 3 envs x 8 cars on small-circle, 64 rays, a roster of per-car nets (with rival inputs, without) and a bundled
    driver: rollout of 50 steps three times against a twin stepped through the host by the model."""
    assert "closed loop ok" in run_child("closed_loop", shape=shape)


@pytest.mark.gpu
def test_net_slot_with_rival_inputs_sees_what_an_agent_is_given():
    """roster ["agent", "net0", "fast"] against ["agent", "agent", "fast"] whose second agent is the model on obs, state, frame and rival
    of the call before: n_rivals 3, lookahead 3, random starts, 40 calls with auto-resets; again with the env's own rivals off and with
    n_rivals 1 in the env."""
    assert "train to deploy ok" in run_child("train_to_deploy")


@pytest.mark.gpu
def test_multitrack_roster_with_the_dynamics_table_on():
    """["small-circle", "circle"], 3 cars per env, net0 (rivals + frame) and net1 (neither) among bundled drivers, dynamics on, against a
    twin stepped through the host; an env on track 1 uses track 1's path for every mate's search."""
    assert "multitrack ok" in run_child("multitrack")


@pytest.mark.gpu
def test_collect_records_the_wider_inputs():
    """T = 12 with noise, next_inputs and action_repeat 2, two agents and a bundled car per env, episode ends inside the window: the
    outputs and the handle equal 12 step calls fed action[t]; inputs[t] and next_inputs[t] are the model's vectors."""
    assert "collect ok" in run_child("collect")


@pytest.mark.gpu
def test_device_setter_and_getters_on_a_rival_network():
    assert "device setter ok" in run_child("device_setter")


@pytest.mark.gpu
def test_errors_leave_a_defined_slot_in_force():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_launches_without_a_rival_slot_run_the_kernels_they_ran():
    assert "no rival slot ok" in run_child("no_rival_slot")
