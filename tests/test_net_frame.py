"""Network drivers with frame inputs (include/ftgp.h: ftgp_set_net_frame / ftgp_get_net_frame; net.NetSpec(frame=, lookahead=,
lookahead_stride=); DeviceVecEnv follows the spec).

CPU: the struct and the binding; NetSpec's checks, which run before the library is loaded, and its behaviour; the shipped element
operations (csrc/ftgp_frame.h and csrc/ftgp_net.h, compiled for the host by tools/net_check.cpp --frame, also under the address and
undefined-behaviour sanitizers) against the model of the header's text (tests/net_frame_model.py = net_model + frame_model), bit for
bit, on paths and poses that reach every branch of the frame row.

GPU: every scenario in a fresh child process (tests/net_frame_child.py), equality to the bit with the model throughout.
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
from tests import net_frame_model as nfm
from tests import net_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "net_frame_child.py")
run_child = functools.partial(children.run_child, CHILD, timeout=300)


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_struct_and_binding():
    from ft_grandprix_amd import capi
    assert ctypes.sizeof(capi.FtgpNetFrame) == 16
    assert [(n, getattr(capi.FtgpNetFrame, n).offset) for n, _ in capi.FtgpNetFrame._fields_] == [("enabled", 0), ("n_ahead", 4), ("stride", 8), ("reserved", 12)]
    assert ctypes.sizeof(capi.FtgpNetDesc) == 68                     # unchanged
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for name in ("set_net_frame", "get_net_frame"):
        assert name in capi.API_SYMBOLS and lib.has(name), name
        assert lib.fn(name).argtypes is not None, name
        assert f"int ftgp_{name}(FtgpEnv *env, int slot, " in header, name
    assert len(lib.fn("set_net_frame").argtypes) == 5 and len(lib.fn("get_net_frame").argtypes) == 3
    assert "typedef struct FtgpNetFrame {" in header
    for method in ("set_net", "net", "net_frame", "get_net"):
        assert callable(getattr(capi.Env, method))
    # the handle-free checks: net_desc's return shape is what it was
    net = nfm.random_net(np.random.default_rng(1), (8,), n_beams=12, lookahead=3, lookahead_stride=2, pool=4, max_range=3.0, beam_first=2)
    out = capi.net_desc(net["layers"], **nfm.fields(net))
    assert len(out) == 2 and isinstance(out[0], capi.FtgpNetDesc) and out[1].size == 8 * 27 + 8 + 2 * 8 + 2
    f = capi.net_frame(False, 3, 2)
    assert (f.enabled, f.n_ahead, f.stride, f.reserved) == (1, 3, 2, 0)


def no_load():
    raise AssertionError("the library was loaded before the arguments were checked")


def spec_of(net):
    from ft_grandprix_amd.net import NetSpec
    return NetSpec(net["layers"], **nfm.fields(net))


def small_spec(n_beams=12, hidden=(8,), **frame):
    from ft_grandprix_amd.net import NetSpec
    look = frame.get("lookahead", 0)
    look = look if isinstance(look, int) and look > 0 else 0        # (a refused value: any width will do, the fields are checked first)
    width0 = n_beams + 5 + ((4 + 2 * look) if (frame.get("frame") or look > 0) else 0)
    net = nm.random_net(np.random.default_rng(1), (width0, *hidden, 2), pool=4, max_range=3.0, beam_first=2, use_state=True)
    net["n_beams"] = n_beams
    return NetSpec(net["layers"], **{**nfm.fields(net), **frame})


@pytest.mark.parametrize("frame", [dict(lookahead=17), dict(frame=True, lookahead_stride=0), dict(frame=True, lookahead_stride=51),
                                   dict(lookahead_stride=0), dict(lookahead=-1), dict(frame=True, lookahead=1.5)])
def test_net_spec_refuses_bad_frame_fields(frame, monkeypatch):
    from ft_grandprix_amd import capi
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError):
        small_spec(**frame)


def test_net_spec_refuses_257_inputs_reached_through_the_frame(monkeypatch):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.net import NetSpec
    monkeypatch.setattr(capi, "load", no_load)
    z = lambda *s: np.zeros(s, dtype=np.float32)                    # noqa: E731
    kw = dict(pool=4, max_range=8.0, beam_first=42, use_state=True)
    NetSpec([(z(2, 256), z(2))], n_beams=215, lookahead=16, **kw)   # 215 + 5 + 36 = 256: the limit
    with pytest.raises(ValueError, match="257"):
        NetSpec([(z(2, 257), z(2))], n_beams=216, lookahead=16, **kw)
    NetSpec([(z(2, 221), z(2))], n_beams=216, **kw)                 # the same beams without the frame are fine
    with pytest.raises(ValueError):
        NetSpec([(z(2, 221), z(2))], n_beams=216, lookahead=16, **kw)       # the first layer must be as wide as the true n_in


def test_net_spec_with_frame_inputs(tmp_path, monkeypatch):
    from ft_grandprix_amd import capi, net
    monkeypatch.setattr(capi, "load", no_load)
    spec = small_spec(lookahead=3)
    assert spec.frame is True and (spec.lookahead, spec.lookahead_stride) == (3, 1)
    assert spec.n_in == 12 + 5 + 4 + 6 and spec.widths == (27, 8, 2) and spec.widths[0] == spec.n_in
    assert spec.flat_params().size == 8 * 27 + 8 + 2 * 8 + 2
    fields = spec.input_fields()
    assert (fields["frame"], fields["lookahead"], fields["lookahead_stride"]) == (True, 3, 1)
    only_fixed = small_spec(frame=True)
    assert only_fixed.n_in == 12 + 5 + 4 and only_fixed.lookahead == 0
    assert small_spec().n_in == 17 and small_spec().frame is False
    # two specs that differ only in the stride cannot replace one another through the device setter
    other = small_spec(lookahead=3, lookahead_stride=2)
    assert other.widths == spec.widths and other.shape_key() != spec.shape_key()
    assert small_spec(lookahead=3).shape_key() == spec.shape_key()
    # the npz round trip
    other.save(tmp_path / "frame.npz")
    back = net.load(tmp_path / "frame.npz")
    assert back.input_fields() == other.input_fields() and back.shape_key() == other.shape_key()
    assert (back.frame, back.lookahead, back.lookahead_stride) == (True, 3, 2)
    np.testing.assert_array_equal(back.flat_params(), other.flat_params())
    # a file written before the frame inputs existed: none of the three keys, the frame is off
    plain = small_spec()
    plain.save(tmp_path / "new.npz")
    with np.load(tmp_path / "new.npz") as z:
        old = {k: z[k] for k in z.files if k not in ("frame", "lookahead", "lookahead_stride")}
    assert len(old) == len(np.load(tmp_path / "new.npz").files) - 3
    np.savez(tmp_path / "old.npz", **old)
    back = net.load(tmp_path / "old.npz")
    assert back.frame is False and back.lookahead == 0 and back.lookahead_stride == 1 and back.shape_key() == plain.shape_key()
    # from_torch
    import torch
    module = torch.nn.Sequential(torch.nn.Linear(29, 8), torch.nn.Tanh(), torch.nn.Linear(8, 2), torch.nn.Tanh())
    t = net.from_torch(module, pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True, frame=True, lookahead=4, lookahead_stride=5)
    assert t.widths == (29, 8, 2) and (t.frame, t.lookahead, t.lookahead_stride) == (True, 4, 5)
    with pytest.raises(ValueError):
        net.from_torch(module, pool=4, max_range=3.0, beam_first=2, n_beams=12, use_state=True, lookahead=3)


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
    tmp = tmp_path_factory.mktemp("net_frame")
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


def run_harness(harness, tmp_path, name, net, n_rays, scans, pose, ctrl, path):
    """(inputs float32 [n, n_in], controls float64 [n, 2]) of tools/net_check --frame."""
    n_cars, flat = len(pose), nfm.flat_params(net)
    widths = [W.shape[0] for W, _ in net["layers"]] + [0] * (4 - len(net["layers"]))
    src, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([n_rays, n_cars, net["pool"], net["beam_first"], net["n_beams"], int(net["use_state"]), len(net["layers"]), *widths,
                  nm.ACT[net["hidden_act"]], nm.ACT[net["out_act"]], flat.size], dtype=np.int32).tofile(f)
        np.array([net["max_range"], *net["out_scale"], *net["out_offset"]], dtype=np.float32).tofile(f)
        np.array([int(net["frame"]), net["lookahead"], net["lookahead_stride"]], dtype=np.int32).tofile(f)
        flat.tofile(f); np.ascontiguousarray(scans, dtype=np.float32).tofile(f)
        np.stack([pose[:, 3], pose[:, 6], pose[:, 7], pose[:, 8], pose[:, 12], ctrl[:, 0], ctrl[:, 1], pose[:, 0], pose[:, 1]], axis=1).tofile(f)
        np.ascontiguousarray(path, dtype=np.float64).tofile(f)
    r = subprocess.run([harness, "--frame", str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w = nfm.n_in(net)
    assert r.stdout.count("inputs") == n_cars and r.stdout.count("speed") == n_cars
    raw = open(out, "rb").read()
    assert len(raw) == 4 * n_cars * w + 16 * n_cars
    return np.frombuffer(raw[:4 * n_cars * w], dtype=np.float32).reshape(n_cars, w), np.frombuffer(raw[4 * n_cars * w:], dtype=np.float64).reshape(n_cars, 2)


def test_the_pose_list_reaches_the_branches_it_names():
    """The poses are what net_frame_model.pose_list says they are, by the model of the header's text."""
    for which, path in nfm.paths().items():
        pose = nfm.pose_list(path, which)
        _, s, off, a, c = fm.frame_rows64(path, pose)
        x, y = pose[:, 0], pose[:, 1]
        A, B = fm._segment(path, (c + 99) % 100, x, y), fm._segment(path, c, x, y)
        assert c[0] == 5 and A["g2"][0] == 0.0 and B["g2"][0] == 0.0 and a[0] == 5, which      # on a point: B on the tie
        assert c[1] == 25 and A["g2"][1] == B["g2"][1] > 0 and a[1] == 25, which                  # outside the bend: B wins the tie
        assert c[2] == 25 and A["g2"][2] < B["g2"][2] and a[2] == 24, which                       # inside: A
        assert c[3] == 0 and a[3] == 99 and c[4] == 99, (which, c[:5], a[:5])
        assert c[5] >= 64 and c[6] >= 64 and off[9] and not off[:9].any(), which
        if which != "square":
            assert c[7] == 10 and a[7] in (9, 10), which                                          # the first of the two equal points
            B10 = fm._segment(path, np.array([10]), x[7:8], y[7:8])
            assert B10["L2"][0] == 1.0 and B10["t"][0] == 0.0                                     # L2 == 0 took the replacement
        if which == "skew":
            assert a[10] == 99 and s[10] == 0.0                                                   # a = 99, t = 1: s = 100 wraps


@pytest.mark.parametrize("which", ["square", "dup", "skew"])
def test_host_harness_equals_the_model(harness, tmp_path, which):
    path = nfm.paths()[which]
    pose = nfm.pose_list(path, which)
    rng = np.random.default_rng(31)
    n_rays = 64
    ctrl = np.stack([rng.uniform(0, 7, len(pose)), rng.uniform(-1, 1, len(pose))], axis=1)
    base = dict(pool=4, max_range=3.0, beam_first=2, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
    for k, shape in enumerate([dict(lookahead=0), dict(lookahead=4, lookahead_stride=1), dict(lookahead=16, lookahead_stride=50),
                               dict(lookahead=16, lookahead_stride=7), dict(lookahead=3, lookahead_stride=2, use_state=False),
                               dict(frame=False)]):
        net = nfm.random_net(rng, (9,), n_beams=12, **{**base, **shape})
        scans = nm.eval_scans(rng, len(pose), n_rays, net["max_range"])
        got_x, got_u = run_harness(harness, tmp_path, f"{which}{k}", net, n_rays, scans, pose, ctrl, path)
        want_u, want_x = nfm.evaluate(net, scans, pose, ctrl, path)
        np.testing.assert_array_equal(got_x.view(np.int32), want_x.view(np.int32), err_msg=f"{which}, {shape}: inputs")
        np.testing.assert_array_equal(got_u, want_u, err_msg=f"{which}, {shape}: controls")
        assert np.abs(want_u).max() > 0
        if net["frame"]:                                             # the look-ahead wrapped past index 99 where the shape says so
            a = fm.frame_rows64(path, pose)[3]
            if net["lookahead"] == 16:
                assert ((a + 1 + 15 * net["lookahead_stride"]) >= 100).all()


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_policy_eval_equals_the_model_and_the_inputs_equal_the_frame_rows():
    """set_pose puts the pose list on the open-field square and skew tracks (8 rays, one layer): ftgp_policy_eval(NET0) equals the model,
    and the act kernel's recorded inputs end with ftgp_get_frames(n_ahead, stride) to the bit.  Shapes: a frame block across lanes
    63 / 64, n_in = 256 with lookahead 16 at 1344 rays, frame with lookahead 0, no state inputs; a finished car gets (0, 0) with its
    inputs still recorded."""
    assert "policy_eval ok" in run_child("policy_eval")


@pytest.mark.gpu
def test_closed_loop_in_one_launch_equals_the_twin_driven_by_the_model():
    """19 envs on small-circle, 64 rays, rollout("net0", 50) three times against a twin stepped through the host by the model."""
    assert "closed loop ok" in run_child("closed_loop")


@pytest.mark.gpu
def test_net_slot_with_frame_inputs_sees_what_an_agent_is_given():
    """roster ["agent", "net0"] against ["agent", "agent"] whose second agent is the model on obs, state and frame of the call before:
    track_frame, lookahead 3, stride 2, random starts, 40 calls with auto-resets; and again with the env's own frame off."""
    assert "train to deploy ok" in run_child("train_to_deploy")


@pytest.mark.gpu
def test_multitrack_roster_with_the_dynamics_table_on():
    """["small-circle", "circle"], 3 cars per env, net0 (frame) and net1 (no frame) among bundled drivers, dynamics on: MULTI x TRACKS x
    DYN against a twin stepped through the host; an env on track 1 uses track 1's path."""
    assert "multitrack ok" in run_child("multitrack")


@pytest.mark.gpu
def test_collect_records_the_wider_inputs():
    """T = 12 with noise, next_inputs and action_repeat 2 on a frame network: the outputs and the handle equal 12 step calls fed
    action[t], inputs[t] the model's vector on the rows of the step before; with action_repeat 1, no noise and no episode end a
    collected agent moves like rollout("net0", T)."""
    assert "collect ok" in run_child("collect")


@pytest.mark.gpu
def test_device_setter_and_getters_on_a_frame_network():
    assert "device setter ok" in run_child("device_setter")


@pytest.mark.gpu
def test_errors_leave_a_defined_slot_in_force():
    assert "errors ok" in run_child("errors")


@pytest.mark.gpu
def test_launches_without_a_frame_slot_run_the_kernels_they_ran():
    assert "no frame slot ok" in run_child("no_frame_slot")
