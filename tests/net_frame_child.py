"""Child process of tests/test_net_frame.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/net_frame_child.py <scenario> [json options]

The criterion throughout: what the library computes with a network driver that has frame inputs (ftgp_set_net_frame) equals, bit for
bit, what the model of the header's text (tests/net_frame_model.py = net_model + frame_model) computes from the same scans and
records -- evaluated on the host and fed back as host controls or actions to a twin that knows nothing of networks.
"""
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: one HIP runtime per process)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402
from tests import collect_model as cmod  # noqa: E402
from tests import frame_model as fm  # noqa: E402
from tests import helpers  # noqa: E402
from tests import net_frame_model as nfm  # noqa: E402
from tests import net_model as nm  # noqa: E402
from tests.collect_child import Buffers, Twin, ext_cars, records  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
DEV = "cuda"
LOOP = dict(n_rays=64, spawn_mode=1, seed=5)
# a driver for 64 rays: beams 2 .. 13 of pool 4, the state and the frame; speed in [0.5, 2.5], steering in [-0.5, 0.5]
DRIVER = dict(pool=4, max_range=3.0, beam_first=2, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
WIDE = ((-1e30, 1e30), (-1e30, 1e30))
FIELD_SHIFT = np.array([8.0, -24.0])                 # the dyadic squares of tests/frame_model.py, moved into the open field


def set_net(env, slot, net):
    env.set_net(slot, net["layers"], **nfm.fields(net))


def driver_net(seed, hidden=16, n_beams=12, **over):
    return nfm.random_net(np.random.default_rng(seed), (hidden,), n_beams=n_beams, **{**DRIVER, **over})


def spec_of(net):
    from ft_grandprix_amd.net import NetSpec
    return NetSpec(net["layers"], **nfm.fields(net))


def read_back(g):
    return dict(lidar=g.lidar(), pose=g.pose(), progress=g.progress(), ctrl=g.ctrl(), steps=g.steps())


def assert_equal_state(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def paths_of(path, cars):
    return [path[c] for c in cars] if isinstance(path, list) else path


def host_step(twin, nets_of_car, path, bundled=None):
    """One step of a twin through the host: every car's controls from the model of its network on lidar() + pose() + get_ctrl() and
    the path of its track -- or, for a car without one, from policy_eval of its bundled driver -- then set_ctrl and step(1)."""
    scans, pose, ctrl = twin.lidar(), twin.pose(), twin.ctrl()
    finished = twin.progress()[:, 4] != 0
    u = twin.policy_eval("per_car", scans) if bundled else np.zeros((twin.n_cars, 2))
    for net, cars in nets_of_car:
        u[cars] = nfm.evaluate(net, scans[cars], pose[cars], ctrl[cars], paths_of(path, cars), finished[cars])[0]
    twin.set_ctrl(u)
    twin.step(1)


def is_net_kernel(name):
    return name.count(",") == 5 and name.endswith("true>")


def recorded_inputs(g, net, slot=0):
    """inputs[0] of a one-decision ftgp_collect_device call: what the act kernel wrote down at the records as they stand, with mean and
    action ([n_envs, 1, .]): one car per env, an agent."""
    buf = Buffers(1, g.n_envs, 1, nfm.n_in(net))
    buf.collect(g, 1, slot=slot, clip=WIDE)
    torch.cuda.synchronize()
    out = buf.host()
    return out["inputs"][0], out["mean"][0], out["action"][0]


def eval_and_record(g, net, path, rng, what, slot=0, finished=False):
    """At the records as they stand (one car per env, every car an agent): ftgp_policy_eval of the slot against the model; the act kernel's
    inputs against the model's vector, and their tail against ftgp_get_frames with the slot's n_ahead and stride."""
    scans = nm.eval_scans(rng, g.n_cars, g.n_rays, net["max_range"])
    pose, ctrl = g.pose(), g.ctrl()
    fin = g.progress()[:, 4] != 0
    assert fin.all() == finished and fin.any() == finished
    want_u, want_x = nfm.evaluate(net, scans, pose, ctrl, path, fin)
    got_u = g.policy_eval(f"net{slot}", scans)
    np.testing.assert_array_equal(got_u, want_u, err_msg=f"{what}: controls")
    if finished:
        np.testing.assert_array_equal(got_u, 0.0)
        assert np.abs(nfm.evaluate(net, scans, pose, ctrl, path)[0]).max() > 0, "the network itself would have proposed something"
    else:
        assert np.abs(want_u).max() > 0, what
    g.set_ctrl(ctrl)                                             # (policy_eval stored its controls: the state inputs)
    w = nfm.n_frame(net)
    frames = g.get_frames(net["lookahead"], net["lookahead_stride"]) if w else None
    x, mean, action = recorded_inputs(g, net, slot)              # (policy_eval left `scans` as the cars' ranges)
    cmod.assert_same_bits(x[:, 0], want_x, f"{what}: the act kernel's inputs")
    if w:
        cmod.assert_same_bits(x[:, 0, -w:], frames, f"{what}: the inputs' tail against ftgp_get_frames")
        cmod.assert_same_bits(frames, fm.frame_rows(path, pose, net["lookahead"], net["lookahead_stride"]), f"{what}: ftgp_get_frames against the model")
    if finished:
        assert (mean == 0).all() and (action == 0).all(), f"{what}: a finished car reads (0, 0)"
    else:
        np.testing.assert_array_equal(action[:, 0].astype(np.float64), want_u, err_msg=f"{what}: the collected action")


def policy_eval(opt):
    lib = capi.load()
    rng = np.random.default_rng(3)
    io = dict(max_episode_steps=0, action_repeat=1, auto_reset=False)
    # the pose list on the open-field squares and the skew track: 8 rays, one layer
    tracks = {"square": fm.square_path() + FIELD_SHIFT, "dup": fm.square_path(duplicate=10) + FIELD_SHIFT, "skew": fm.skew_path()}
    small = dict(pool=1, max_range=2.5, beam_first=1, hidden_act="identity", out_act="identity", out_scale=(1.0, 0.5), out_offset=(0.5, 0.1))
    for which, path in tracks.items():
        poses = nfm.pose_list(path, which)
        t = dataclasses.replace(helpers.open_field(200), path=path, name=which)
        with capi.Env(lib, t, n_envs=len(poses), cars_per_env=1, n_rays=8) as g:
            g.device_io_config(["agent"], **io)
            base = g.pose()
            base[:, [0, 1, 3, 6, 7, 8, 12]] = poses[:, [0, 1, 3, 6, 7, 8, 12]]
            for k, shape in enumerate((dict(lookahead=16, lookahead_stride=50), dict(lookahead=16, lookahead_stride=7), dict(lookahead=3, lookahead_stride=2),
                                       dict(lookahead=0))):
                net = nfm.random_net(rng, (), n_beams=4, **{**small, **shape})
                set_net(g, k, net)
                g.set_pose(base)
                g.set_ctrl(np.stack([rng.uniform(0, 7, g.n_cars), rng.uniform(-1, 1, g.n_cars)], axis=1))
                np.testing.assert_array_equal(g.pose()[:, :2], poses[:, :2])
                eval_and_record(g, net, path, rng, f"{which}, {shape}", slot=k)
        print(f"policy_eval {which} ok")
    # shapes on small-circle: the frame block across lanes 63 / 64; n_in = 256; frame with lookahead 0; no state inputs
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    wide = dict(pool=10, max_range=10.0, beam_first=14, out_scale=(3.5, 0.6), out_offset=(3.5, 0.0))
    limit = dict(pool=4, max_range=8.0, beam_first=42, gain=2.0)
    shapes = (("straddle", 1080, nfm.random_net(rng, (64, 64), n_beams=58, lookahead=4, **wide)),
              ("limit", 1344, nfm.random_net(rng, (128, 128, 128), n_beams=215, lookahead=16, lookahead_stride=3, **limit)),
              ("fixed only", 1080, nfm.random_net(rng, (37,), n_beams=80, frame=True, hidden_act="relu", **wide)),
              ("no state", 1080, nfm.random_net(rng, (64,), n_beams=61, use_state=False, lookahead=2, lookahead_stride=5, **wide)))
    assert [nfm.n_in(n) for _, _, n in shapes] == [75, 256, 89, 69]
    assert shapes[0][2]["n_beams"] + 5 == 63 and shapes[3][2]["n_beams"] == 61          # blocks that begin at lanes 63 and 61 and cross into register 1
    for what, n_rays, net in shapes:
        with capi.Env(lib, t, n_envs=7, cars_per_env=1, n_rays=n_rays, spawn_mode=1, seed=2) as g:
            g.device_io_config(["agent"], **io)
            set_net(g, 0, net)
            pose, ctrl = nm.eval_records(rng, g.n_cars)
            pose[:, :3] = g.pose()[:, :3]
            pose[:, :2] += rng.uniform(-0.3, 0.3, (g.n_cars, 2))
            g.set_pose(pose); g.set_ctrl(ctrl)
            eval_and_record(g, net, path, rng, what)
        print(f"policy_eval {what} ok")
    # finished cars get (0, 0) before the network is looked at, and their inputs are recorded all the same
    net = driver_net(7, lookahead=3, lookahead_stride=2)
    with capi.Env(lib, t, n_envs=3, cars_per_env=1, n_rays=64, lap_target=0) as g:
        g.device_io_config(["agent"], **io)
        set_net(g, 0, net)
        eval_and_record(g, net, path, rng, "finished", finished=True)
    print("policy_eval ok")


def closed_loop(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    net = driver_net(21, lookahead=4, lookahead_stride=3)
    with capi.Env(lib, t, n_envs=19, **LOOP) as g, capi.Env(lib, t, n_envs=19, **LOOP) as o:
        set_net(g, 0, net)
        everyone = [(net, np.arange(o.n_cars))]
        for launch in range(3):
            g.rollout("net0", 50)
            for _ in range(50):
                host_step(o, everyone, path)
            assert_equal_state(read_back(g), read_back(o), f"closed loop, launch {launch}")
        assert is_net_kernel(g.kernel_name()), g.kernel_name()
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
    print("closed loop ok")


def train_to_deploy(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    L, S = 3, 2
    net = driver_net(41, lookahead=L, lookahead_stride=S)
    kw = dict(n_envs=7, n_rays=64, cars_per_env=2, action_repeat=1, max_episode_steps=15, scan_pool=net["pool"], scan_max_range=net["max_range"],
              state=True, spawn_mode=1, seed=9, random_start=True, start_lateral=0.6, start_yaw_jitter=0.2)
    frame_kw = dict(track_frame=True, lookahead=L, lookahead_stride=S)
    lo, hi = net["beam_first"], net["beam_first"] + net["n_beams"]
    for what, a_kw in (("the env's frame as the slot's", frame_kw), ("the env's frame off", {})):
        a = DeviceVecEnv("small-circle", roster=["agent", "net0"], nets={0: spec_of(net)}, **kw, **a_kw)
        b = DeviceVecEnv("small-circle", roster=["agent", "agent"], **kw, **frame_kw)
        assert a.track_frame == bool(a_kw) and b.track_frame
        a.reset(); b.reset()
        obs_b, state_b, frame_b = b.obs.clone(), b.state.clone(), b.frame.clone()
        resets = 0
        for call in range(40):
            shared = torch.tensor([1.5 + 0.5 * np.sin(0.3 * call), 0.3 * np.cos(0.2 * call)], dtype=torch.float32, device=a.device)
            x = np.concatenate([obs_b[:, 1, lo:hi].cpu().numpy(), state_b[:, 1, :5].cpu().numpy(), frame_b[:, 1].cpu().numpy()], axis=1)
            assert x.shape[1] == nfm.n_in(net)
            u = nm.evaluate(net, None, inputs=x)
            act_a = shared.expand(a.n_envs, 1, 2).contiguous()
            act_b = torch.cat([act_a, torch.from_numpy(u.astype(np.float32)).to(a.device)[:, None, :]], dim=1).contiguous()
            oa, ra, ta, tra, ia = a.step(act_a)
            ob, rb, tb, trb, ib = b.step(act_b)
            where = f"{what}, call {call}"
            assert torch.equal(oa[:, 0], ob[:, 0]) and torch.equal(ra[:, 0], rb[:, 0]) and torch.equal(ia["state"][:, 0], ib["state"][:, 0]), where
            if a_kw:
                assert torch.equal(ia["frame"][:, 0], ib["frame"][:, 0]), where
            assert torch.equal(ta, tb) and torch.equal(tra, trb), where
            np.testing.assert_array_equal(a.env.pose(), b.env.pose(), err_msg=where)
            np.testing.assert_array_equal(a.env.lidar(), b.env.lidar(), err_msg=where)
            resets += int((ta | tra).sum())
            obs_b, state_b, frame_b = ob.clone(), ib["state"].clone(), ib["frame"].clone()
        assert resets >= 7, "no auto-reset happened"
        assert is_net_kernel(a.env.kernel_name()), a.env.kernel_name()
        a.close(); b.close()
        print(f"train to deploy, {what}: ok")
    print("train to deploy ok")


def multitrack(opt):
    lib = capi.load()
    tracks = [load_track("small-circle"), load_track("circle")]
    counts, cpe = (3, 4), 3
    n = sum(counts)
    names = ["net0", "fast", "net1"]
    nets = [driver_net(51, lookahead=5, lookahead_stride=4), driver_net(52, hidden=37, hidden_act="relu", frame=False)]
    assert nets[0]["frame"] and not nets[1]["frame"]
    path = fm.env_paths([np.asarray(t.path, dtype=np.float64) for t in tracks], counts, cpe)
    kw = dict(n_envs=n, envs_per_track=counts, cars_per_env=cpe, **LOOP)
    with capi.Env(lib, tracks, **kw) as g, capi.Env(lib, tracks, **kw) as twin:
        rows = g.base_dynamics() * np.random.default_rng(8).uniform(helpers.DYN_LO, helpers.DYN_HI, (n, cpe, 8))
        for e in (g, twin):
            e.set_dynamics(rows)
        for s, net in enumerate(nets):
            set_net(g, s, net)
        g.set_car_policies(names)
        twin.set_car_policies([x if not x.startswith("net") else "lobotomy" for x in names])
        slot = np.array([int(x[3:]) if x.startswith("net") else -1 for x in names] * n)
        of_car = [(nets[s], np.flatnonzero(slot == s)) for s in range(2)]
        # an env on track 1 must use track 1's path: the model with track 0's path for those cars says something else
        on_1 = np.flatnonzero((slot == 0) & (np.arange(n * cpe) >= counts[0] * cpe))
        x1 = nfm.inputs(nets[0], g.lidar()[on_1], g.pose()[on_1], g.ctrl()[on_1], paths_of(path, on_1))
        x0 = nfm.inputs(nets[0], g.lidar()[on_1], g.pose()[on_1], g.ctrl()[on_1], path[0])
        assert not np.array_equal(x0, x1)
        g.rollout("per_car", 30)
        for _ in range(30):
            host_step(twin, of_car, path, bundled=True)
        assert_equal_state(read_back(g), read_back(twin), "multi-track roster with dynamics")
        name = g.kernel_name()
        assert name == "ftgp_step_kernel<true, false, true, true, true, true>", name
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
    print("multitrack ok")


def model_rows(net, rb, path, std, noise, lo, hi):
    """(x, mean, action) [n_envs, n_ext, .] of the model on a twin's read-backs: collect_model's decision on the wider input vector."""
    n, k = rb["finished"].shape
    flat = lambda a: a.reshape((n * k,) + a.shape[2:])          # noqa: E731
    x = nfm.inputs(net, flat(rb["scans"]), flat(rb["pose"]), flat(rb["ctrl"]), path)
    y = nm.forward(x, net["layers"], net["hidden_act"], net["out_act"])
    m = cmod.mean(y, net["out_scale"], net["out_offset"])
    a = cmod.action(m, std, None if noise is None else flat(noise), lo, hi)
    fin = flat(rb["finished"])[:, None]
    m, a = np.where(fin, np.float32(0), m).astype(np.float32), np.where(fin, np.float32(0), a).astype(np.float32)
    return x.reshape(n, k, -1), m.reshape(n, k, 2), a.reshape(n, k, 2)


def collect(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    net = driver_net(61, lookahead=3, lookahead_stride=2)
    roster, n_envs, T = ["agent", "fast", "agent"], 3, 12
    io = dict(max_episode_steps=7, action_repeat=2, auto_reset=True)
    envs = []
    for _ in range(2):
        e = capi.Env(lib, t, n_envs=n_envs, cars_per_env=len(roster), n_rays=64, spawn_mode=1, seed=5)
        e.device_io_config(roster, **io)
        envs.append(e)
    g, tw = envs
    set_net(g, 0, net)
    cars = ext_cars(g, roster)
    n, k = cars.shape
    std, clip = (0.3, 0.2), ((0.0, 6.0), (-0.5, 0.5))
    lo, hi = (clip[0][0], clip[1][0]), (clip[0][1], clip[1][1])
    noise = np.random.default_rng(7).standard_normal((T, n, k, 2)).astype(np.float32)
    nz = torch.from_numpy(noise).to(DEV)
    buf = Buffers(T, n, k, nfm.n_in(net), next_inputs=True)
    buf.collect(g, T, std=std, clip=clip, noise=nz.data_ptr())
    torch.cuda.synchronize()
    out = buf.host()
    assert out["inputs"].shape[-1] == 12 + 5 + 4 + 6
    twin = Twin(tw, roster, 64)
    ended_total = 0
    for s in range(T):
        rb = twin.read()
        x, m, a = model_rows(net, rb, path, std, noise[s], lo, hi)
        cmod.assert_same_bits(out["inputs"][s], x, f"inputs[{s}]")
        cmod.assert_same_bits(out["mean"][s], m, f"mean[{s}]")
        cmod.assert_same_bits(out["action"][s], a, f"action[{s}]")
        reward, term, trunc = twin.step(out["action"][s])
        cmod.assert_same_bits(out["reward"][s], reward, f"reward[{s}]")
        np.testing.assert_array_equal(out["terminated"][s], term, err_msg=f"terminated[{s}]")
        np.testing.assert_array_equal(out["truncated"][s], trunc, err_msg=f"truncated[{s}]")
        ended = (term | trunc).astype(bool)
        ended_total += int(ended.sum())
        after = model_rows(net, twin.read(), path, std, None, lo, hi)[0]          # what the next decision sees
        keep = ~ended
        cmod.assert_same_bits(out["next_inputs"][s][keep], after[keep], f"next_inputs[{s}] without a reset")
        if ended.any():
            assert not cmod.same_bits(out["next_inputs"][s][ended], after[ended]), f"next_inputs[{s}]: the rows before the reset"
    assert ended_total >= n_envs, "no episode ended"
    np.testing.assert_array_equal(records(g), records(tw), err_msg="the env-state records at the end")
    for name, p, q in (("lidar", g.lidar(), tw.lidar()), ("pose", g.pose(), tw.pose()), ("ctrl", g.ctrl(), tw.ctrl()), ("steps", g.steps(), tw.steps())):
        np.testing.assert_array_equal(p, q, err_msg=f"{name} at the end")
    g.close(); tw.close()
    # action_repeat 1, no noise, no episode end: a collected agent moves like rollout("net0", T)
    kw = dict(n_envs=5, n_rays=64, spawn_mode=1, seed=5)
    T = 20
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as r:
        set_net(g, 0, net); set_net(r, 0, net)
        g.device_io_config(["agent"], max_episode_steps=0, action_repeat=1, auto_reset=True)
        buf = Buffers(T, 5, 1, nfm.n_in(net))
        buf.collect(g, T, clip=WIDE)
        torch.cuda.synchronize()
        r.rollout("net0", T)
        np.testing.assert_array_equal(g.pose(), r.pose(), err_msg="pose against ftgp_rollout(net0)")
        np.testing.assert_array_equal(g.lidar(), r.lidar(), err_msg="lidar against ftgp_rollout(net0)")
        out = buf.host()
        assert not out["terminated"].any() and not out["truncated"].any()
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
    print("collect ok")


def device_setter(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    shape = dict(lookahead=2, lookahead_stride=9)
    net_a, net_b = driver_net(61, **shape), driver_net(62, **shape)
    rng = np.random.default_rng(6)
    with capi.Env(lib, t, n_envs=5, **LOOP) as g, capi.Env(lib, t, n_envs=5, **LOOP) as h:
        set_net(g, 0, net_a); set_net(h, 0, net_a)
        flat_b = torch.from_numpy(nfm.flat_params(net_b)).to(DEV)
        assert flat_b.numel() == 16 * 25 + 16 + 2 * 16 + 2
        stream = torch.cuda.current_stream().cuda_stream
        # a replacement enqueued between two launches is in force for the second and not for the first
        g.rollout("net0", 10)
        g.set_net_device(0, flat_b.data_ptr(), stream)
        g.rollout("net0", 10)
        h.rollout("net0", 10)
        first = read_back(h)
        set_net(h, 0, net_b)
        h.rollout("net0", 10)
        assert_equal_state(read_back(g), read_back(h), "device setter between two launches")
        assert not np.array_equal(first["pose"], read_back(h)["pose"])
        scans = nm.eval_scans(rng, g.n_cars, 64, net_b["max_range"])
        ctrl = g.ctrl()
        want = nfm.evaluate(net_b, scans, g.pose(), ctrl, path)[0]
        np.testing.assert_array_equal(g.policy_eval("net0", scans), want)
        # ftgp_get_net and ftgp_get_net_frame return what was set: the first layer has the true n_in columns
        for env in (g, h):
            d, layers, frame = env.get_net(0)
            assert (d.pool, d.beam_first, d.n_beams, d.use_state, d.n_layers) == (4, 2, 12, 1, 2) and list(d.width) == [16, 2, 0, 0] and d.reserved == 0
            assert frame == dict(frame=True, lookahead=2, lookahead_stride=9), frame
            assert layers[0][0].shape == (16, 25)
            for (W, b), (W0, b0) in zip(layers, net_b["layers"]):
                np.testing.assert_array_equal(W, W0); np.testing.assert_array_equal(b, b0)
        # a host pointer is refused before anything is enqueued
        host = np.zeros(1000, dtype=np.float32)
        assert g.lib.fn("set_net_device")(g.h, None, 0, host.ctypes.data) == ERR_ARG
        # a slot without frame inputs reads zeros
        set_net(g, 1, driver_net(63, frame=False))
        assert g.net_frame(1) == dict(frame=False, lookahead=0, lookahead_stride=1)
        f = capi.FtgpNetFrame(enabled=7, n_ahead=7, stride=7, reserved=7)
        assert lib.fn("get_net_frame")(g.h, 1, f) == 0 and (f.enabled, f.n_ahead, f.stride, f.reserved) == (0, 0, 0, 0)
    print("device setter ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    rng = np.random.default_rng(4)
    limit = dict(pool=4, max_range=8.0, beam_first=42)
    net = nfm.random_net(rng, (8,), n_beams=215, lookahead=16, **limit)                  # n_in = 256
    with capi.Env(lib, t, n_envs=2, n_rays=1344, spawn_mode=1, seed=5) as g:
        f0 = capi.FtgpNetFrame()
        assert lib.fn("get_net_frame")(g.h, 0, f0) == ERR_STATE and "not defined" in lib.last_error()
        assert lib.fn("get_net_frame")(g.h, 4, f0) == ERR_ARG and lib.fn("get_net_frame")(g.h, -1, f0) == ERR_ARG
        scans = nm.eval_scans(rng, g.n_cars, 1344, net["max_range"])
        set_net(g, 0, net)
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        want = nfm.evaluate(net, scans, g.pose(), g.ctrl(), path)[0]
        d0, flat = capi.net_desc(net["layers"], **nfm.fields(net))
        big = np.zeros(flat.size + 2 * 64, dtype=np.float32)

        def refused(word, expect=ERR_ARG, slot=0, params=flat, desc=None, **frame):
            d = capi.FtgpNetDesc.from_buffer_copy(d0)
            for k, v in (desc or {}).items():
                setattr(d, k, v)
            f = capi.FtgpNetFrame(**{**dict(enabled=1, n_ahead=16, stride=1, reserved=0), **frame})
            rc = lib.fn("set_net_frame")(g.h, slot, d, f, None if params is None else params.ctypes.data)
            assert rc == expect, (frame, desc, slot, rc, lib.last_error())
            assert word in lib.last_error(), (word, lib.last_error())
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval("net0", scans), want, err_msg=f"slot 0 after {frame} {desc}")
            got = g.net_frame(0)
            assert got == dict(frame=True, lookahead=16, lookahead_stride=1), got
        refused("enabled", enabled=2); refused("enabled", enabled=-1)
        refused("n_ahead", n_ahead=17); refused("n_ahead", n_ahead=-1); refused("stride", stride=0); refused("stride", stride=51)
        refused("n_ahead", enabled=0, n_ahead=17); refused("stride", enabled=0, stride=0)           # checked with the frame off too
        refused("reserved", reserved=1)
        refused("n_in", desc=dict(n_beams=216), params=big)                                           # 216 + 5 + 36 = 257, reached only through the frame
        # ftgp_set_net's own checks, through the new entry
        refused("slot", slot=4); refused("slot", slot=-1); refused("params", params=None)
        refused("pool", desc=dict(pool=5)); refused("reserved", desc=dict(reserved=1)); refused("use_state", desc=dict(use_state=2))
        refused("beam", desc=dict(beam_first=41)); refused("n_layers", desc=dict(n_layers=0))
        # 216 beams without the frame are fine (n_in = 221), into another slot
        d = capi.FtgpNetDesc.from_buffer_copy(d0); d.n_beams = 216
        assert lib.fn("set_net_frame")(g.h, 1, d, None, big.ctypes.data) == 0, lib.last_error()
        assert lib.fn("set_net_frame")(g.h, 1, d, capi.FtgpNetFrame(enabled=0, n_ahead=16, stride=50), big.ctypes.data) == 0, lib.last_error()
        assert g.net_frame(1) == dict(frame=False, lookahead=0, lookahead_stride=1)
    # enabled == 0 and frame == NULL are ftgp_set_net to the letter
    small = driver_net(81, frame=False)
    with capi.Env(lib, t, n_envs=2, cars_per_env=2, **LOOP) as g:
        scans = nm.eval_scans(rng, g.n_cars, 64, small["max_range"])
        d0, flat = capi.net_desc(small["layers"], **nfm.fields(small))
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        want = nm.evaluate(small, scans, g.pose(), g.ctrl())
        assert lib.fn("set_net")(g.h, 0, d0, flat.ctypes.data) == 0
        assert lib.fn("set_net_frame")(g.h, 1, d0, None, flat.ctypes.data) == 0
        assert lib.fn("set_net_frame")(g.h, 2, d0, capi.FtgpNetFrame(enabled=0, n_ahead=5, stride=3), flat.ctypes.data) == 0
        for s in range(3):
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval(f"net{s}", scans), want, err_msg=f"slot {s}")
            assert g.net(s)[1][0][0].shape == (16, 17)
    with capi.Env(lib, t, n_envs=1, n_rays=64, lidar_mode="fakelidar") as f:
        assert lib.fn("set_net_frame")(f.h, 0, d0, capi.FtgpNetFrame(enabled=1, n_ahead=0, stride=1), flat.ctypes.data) == ERR_STATE
    print("errors ok")


def no_frame_slot(opt):
    lib = capi.load()
    t = load_track("small-circle")
    kw = dict(n_envs=4, cars_per_env=3, **LOOP)
    plain = driver_net(71, frame=False)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as fresh:
        set_net(g, 0, plain); set_net(g, 1, driver_net(72, lookahead=4))
        set_net(fresh, 0, plain)
        for e in (g, fresh):
            e.rollout("fast", 30)
        assert g.kernel_name() == fresh.kernel_name() == "ftgp_step_kernel<true, false, false>", (g.kernel_name(), fresh.kernel_name())
        for e in (g, fresh):
            e.rollout("net0", 30)
        net_name = fresh.kernel_name()
        assert g.kernel_name() == net_name and is_net_kernel(net_name), (g.kernel_name(), net_name)
        assert_equal_state(read_back(g), read_back(fresh), "rollout net0 beside a slot with frame inputs")
        for e in (g, fresh):
            e.set_car_policies(["net0", "fast", "lobotomy"])
            e.rollout("per_car", 30)
        assert g.kernel_name() == fresh.kernel_name() and is_net_kernel(g.kernel_name()), (g.kernel_name(), fresh.kernel_name())
        assert_equal_state(read_back(g), read_back(fresh), "a roster with a slot without frame inputs")
        g.rollout("net1", 5)
        assert g.kernel_name() == net_name, g.kernel_name()                # a frame slot has no kernels of its own
    print("no frame slot ok")


SCENARIOS = {"policy_eval": policy_eval, "closed_loop": closed_loop, "train_to_deploy": train_to_deploy, "multitrack": multitrack,
             "collect": collect, "device_setter": device_setter, "errors": errors, "no_frame_slot": no_frame_slot}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
