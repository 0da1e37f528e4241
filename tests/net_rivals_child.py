"""Child process of tests/test_net_rivals.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/net_rivals_child.py <scenario> [json options]

The criterion throughout: what the library computes with a network driver that has rival inputs (ftgp_set_net_rivals) equals, bit for
bit, what the model of the header's text (tests/net_rivals_model.py = net_frame_model + rival_model) computes from the same scans and
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
from tests import net_model as nm  # noqa: E402
from tests import net_rivals_model as nrm  # noqa: E402
from tests import rival_model as rm  # noqa: E402
from tests.collect_child import Buffers, Twin, ext_cars, records  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
DEV = "cuda"
LOOP = dict(n_rays=64, spawn_mode=1, seed=5)
# a driver for 64 rays: beams 2 .. 13 of pool 4, the state, the frame and the rivals; speed in [0.5, 2.5], steering in [-0.5, 0.5]
DRIVER = dict(pool=4, max_range=3.0, beam_first=2, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
WIDE = ((-1e30, 1e30), (-1e30, 1e30))
FIELD_SHIFT = np.array([8.0, -24.0])                 # the dyadic square of tests/frame_model.py, moved into the open field
IO = dict(max_episode_steps=0, action_repeat=1, auto_reset=False)


def set_net(env, slot, net):
    env.set_net(slot, net["layers"], **nrm.fields(net))


def driver_net(seed, hidden=16, n_beams=12, **over):
    return nrm.random_net(np.random.default_rng(seed), (hidden,), n_beams=n_beams, **{**DRIVER, **over})


def spec_of(net):
    from ft_grandprix_amd.net import NetSpec
    return NetSpec(net["layers"], **nrm.fields(net))


def read_back(g):
    return dict(lidar=g.lidar(), pose=g.pose(), progress=g.progress(), ctrl=g.ctrl(), steps=g.steps())


def assert_equal_state(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def is_net_kernel(name):
    return name.count(",") == 5 and name.endswith("true>")


def model_all(net, env, path, scans=None, ctrl=None):
    """(controls, inputs) of the model for EVERY car of the handle as if `net` drove it, at the records as they stand."""
    race = nrm.race_of(env)
    return nrm.evaluate(net, env.lidar() if scans is None else scans, env.pose(), env.ctrl() if ctrl is None else ctrl, path, race,
                        finished=race["finished"] != 0)


def host_step(twin, nets_of_car, path, bundled=None, rows=None):
    """One step of a twin through the host: every car's controls from the model of its network on the records of its whole env -- or,
    for a car without one, from policy_eval of its bundled driver -- then set_ctrl and step(1).  rows: a list that takes the model's
    rival rows (7 slots) of this step."""
    scans, ctrl = twin.lidar(), twin.ctrl()                      # (the controls in force: policy_eval stores its own)
    u = twin.policy_eval("per_car", scans) if bundled else np.zeros((twin.n_cars, 2))
    for net, cars in nets_of_car:
        u[cars] = model_all(net, twin, path, scans, ctrl)[0][cars]
    if rows is not None:
        rows.append(nrm.rival_block(dict(n_rivals=7), twin.pose(), nrm.race_of(twin), path))
    twin.set_ctrl(u)
    twin.step(1)


def recorded_inputs(g, net, slot=0):
    """inputs[0] of a one-decision ftgp_collect_device call, every car an agent: what the act kernel wrote down at the records as they
    stand, with mean and action, [n_cars, .]."""
    cpe = g.n_cars // g.n_envs
    buf = Buffers(1, g.n_envs, cpe, nrm.n_in(net))
    buf.collect(g, 1, slot=slot, clip=WIDE)
    torch.cuda.synchronize()
    out = buf.host()
    flat = lambda a: a[0].reshape((g.n_cars,) + a.shape[3:])          # noqa: E731
    return flat(out["inputs"]), flat(out["mean"]), flat(out["action"])


def eval_and_record(g, net, path, rng, what, slot=0):
    """At the records as they stand (every car an agent): ftgp_policy_eval of the slot against the model; the act kernel's inputs against
    the model's vector, and their tail against ftgp_get_rivals with the slot's n_rivals.  Returns the model's inputs."""
    scans = nm.eval_scans(rng, g.n_cars, g.n_rays, net["max_range"])
    ctrl = g.ctrl()
    fin = g.progress()[:, 4] != 0
    want_u, want_x = model_all(net, g, path, scans)
    got_u = g.policy_eval(f"net{slot}", scans)
    np.testing.assert_array_equal(got_u, want_u, err_msg=f"{what}: controls")
    np.testing.assert_array_equal(got_u[fin], 0.0, err_msg=f"{what}: a finished car reads (0, 0)")
    if not fin.all():
        assert np.abs(want_u).max() > 0, what
    g.set_ctrl(ctrl)                                             # (policy_eval stored its controls: the state inputs)
    w = nrm.n_rival(net)
    rows = g.get_rivals(net["n_rivals"]) if w else None          # (before the collect call, which steps the env)
    x, mean, action = recorded_inputs(g, net, slot)              # (policy_eval left `scans` as the cars' ranges)
    cmod.assert_same_bits(x, want_x, f"{what}: the act kernel's inputs")
    if w:
        cmod.assert_same_bits(x[:, -w:], rows, f"{what}: the inputs' tail against ftgp_get_rivals")
    assert (mean[fin] == 0).all() and (action[fin] == 0).all(), f"{what}: a finished car reads (0, 0)"
    np.testing.assert_array_equal(action[~fin].astype(np.float64), want_u[~fin], err_msg=f"{what}: the collected action")
    return want_x


def put(base, envs, cpe):
    """The pose rows of `envs` (lists of cars in rival_model.hand_scenes()'s format, cpe each) on top of `base`."""
    pose = base.copy()
    for e, cars in enumerate(envs):
        for k, (x, y, q, vx, vy, *_) in enumerate(cars):
            row = pose[e * cpe + k]
            row[0], row[1], row[3], row[6] = x, y, q[0], q[1]
            row[7:] = 0.0
            row[7], row[8] = vx, vy
    return pose


def policy_eval(opt):
    lib = capi.load()
    rng = np.random.default_rng(3)
    # the hand scenes (the cars that race) and random envs on the open-field square: 8 rays, one identity layer
    path = fm.square_path() + FIELD_SHIFT
    t = dataclasses.replace(helpers.open_field(200), path=path, name="square")
    small = dict(pool=1, max_range=2.5, beam_first=1, hidden_act="identity", out_act="identity", out_scale=(1.0, 0.5), out_offset=(0.5, 0.1))
    shapes = (dict(n_rivals=0), dict(n_rivals=1, use_state=False), dict(n_rivals=3, lookahead=2, lookahead_stride=3), dict(n_rivals=7))
    shifted = lambda cars: [(x + FIELD_SHIFT[0], y + FIELD_SHIFT[1], *rest) for x, y, *rest in cars]          # noqa: E731
    seen = dict(padded=0, full=0, g_ties=0, d2_ties=0)
    for cpe in (1, 2, 3, 5, 8):
        envs = []
        for cars in nrm.all_scenes().values():
            racing = shifted([c for c in cars if not c[6]])[:cpe]
            envs.append(racing + nrm.random_env(path, rng, cpe - len(racing)))
        envs += [nrm.random_env(path, rng, cpe) for _ in range(3)]
        with capi.Env(lib, t, n_envs=len(envs), cars_per_env=cpe, n_rays=8, spawn_mode=0) as g:
            g.device_io_config(["agent"] * cpe, **IO)
            placed = put(g.pose(), envs, cpe)
            for k, shape in enumerate(shapes):
                net = nrm.random_net(rng, (), n_beams=4, **{**small, **shape})
                set_net(g, k, net)
                g.set_pose(placed)                               # (again for every shape: the collect call of the one before stepped the env)
                g.eval_progress()
                g.set_ctrl(np.stack([rng.uniform(0, 7, g.n_cars), rng.uniform(-1, 1, g.n_cars)], axis=1))
                if k == 0:                                       # what the envs hold, by the model
                    rows, gg, _, _ = rm.rival_rows64(path, g.pose(), g.progress()[:, 3], g.progress()[:, 4], g.race_steps()[:, 1], cpe, 7)
                    ge = gg.reshape(-1, cpe)
                    seen["g_ties"] += int(((ge[:, :, None] == ge[:, None, :]).sum() - ge.size) // 2)
                    if cpe >= 3:
                        d2 = rows[:, 4::8][:, :cpe - 1] ** 2 + rows[:, 5::8][:, :cpe - 1] ** 2
                        seen["d2_ties"] += int((d2[:, 0] == d2[:, 1]).sum())
                x = eval_and_record(g, net, path, rng, f"square, {cpe} cars, {shape}", slot=k)
                if shape["n_rivals"]:
                    present = x[:, -8 * shape["n_rivals"]:].reshape(g.n_cars, -1, 8)[:, :, rm.PRESENT]
                    seen["padded"] += int((present == 0).sum()); seen["full"] += int((present.sum(axis=1) < cpe - 1).sum())
        print(f"policy_eval square, {cpe} cars ok")
    print(seen)
    assert seen["padded"] > 0 and seen["full"] > 0 and seen["g_ties"] > 0 and seen["d2_ties"] > 0, seen
    # finishers among racing cars, made by teleport: ghosts to the others, their place the one of ftgp_get_winners
    from tests.crowded_model import FINISHERS, finish_by_teleport
    tt, cpe = load_track("track"), 8
    tpath = np.asarray(tt.path, dtype=np.float64)
    with capi.Env(lib, tt, n_envs=2, cars_per_env=cpe, n_rays=8, spawn_mode=0, lap_target=1) as g:
        g.step(1)
        finish_by_teleport((g,), tt, cpe)
        g.device_io_config(["agent"] * cpe, **IO)
        fin = g.progress()[:, 4] != 0
        assert fin.sum() == len(FINISHERS)
        for k, shape in enumerate(shapes):
            net = nrm.random_net(rng, (), n_beams=4, **{**small, **shape})
            set_net(g, k, net)
            x = eval_and_record(g, net, tpath, rng, f"finishers, {shape}", slot=k)
            first = nrm.n_in(net) - nrm.n_rival(net)
            np.testing.assert_array_equal(x[fin, first + rm.PLACE], g.winners().reshape(-1)[fin].astype(np.float32), err_msg="a finished car's place")
            assert (x[fin, first + 2:] == 0).all(), "a finished car has no gaps and no mates"
    print("policy_eval finishers ok")
    # shapes on small-circle, three cars per env: where the block lies among the lanes and registers
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    wide = dict(pool=10, max_range=10.0, beam_first=14, out_scale=(3.5, 0.6), out_offset=(3.5, 0.0))
    four = dict(pool=4, max_range=8.0, beam_first=42, gain=2.0)
    shapes = (("lane 63", 1080, 3, nrm.random_net(rng, (64, 64), n_beams=58, n_rivals=3, **wide)),
              ("lanes 127 / 128", 1080, 3, nrm.random_net(rng, (64,), n_beams=115, n_rivals=2, **four)),
              ("limit", 1344, 3, nrm.random_net(rng, (128, 128, 128), n_beams=155, lookahead=16, lookahead_stride=3, n_rivals=7, **four)),
              ("fixed only", 1080, 3, nrm.random_net(rng, (37,), n_beams=80, n_rivals=0, hidden_act="relu", **wide)),
              ("no state, no frame", 1080, 3, nrm.random_net(rng, (64,), n_beams=61, use_state=False, n_rivals=2, **wide)),
              ("one car per env", 1080, 1, nrm.random_net(rng, (64,), n_beams=58, n_rivals=3, **wide)))
    assert [nrm.n_in(n) for *_, n in shapes] == [91, 140, 256, 89, 81, 91]
    assert shapes[0][3]["n_beams"] + 5 == 63 and shapes[1][3]["n_beams"] + 5 == 120          # blocks at lanes 63 .. 90 and 120 .. 139
    for what, n_rays, cpe, net in shapes:
        with capi.Env(lib, t, n_envs=5, cars_per_env=cpe, n_rays=n_rays, spawn_mode=1, seed=2) as g:
            g.device_io_config(["agent"] * cpe, **IO)
            set_net(g, 0, net)
            pose, ctrl = nm.eval_records(rng, g.n_cars)
            pose[:, :3] = g.pose()[:, :3]
            pose[:, :2] += rng.uniform(-0.3, 0.3, (g.n_cars, 2))
            g.set_pose(pose); g.set_ctrl(ctrl)
            x = eval_and_record(g, net, path, rng, what)
            if cpe == 1:
                np.testing.assert_array_equal(x[:, -28:], np.tile(np.array([1, 1, 0, 0] + [0] * 24, dtype=np.float32), (g.n_cars, 1)))
        print(f"policy_eval {what} ok")
    # every car finished: (0, 0) before the network is looked at, the inputs recorded all the same
    net = driver_net(7, n_rivals=3, lookahead=3, lookahead_stride=2)
    with capi.Env(lib, t, n_envs=3, cars_per_env=3, n_rays=64, lap_target=0) as g:
        g.device_io_config(["agent"] * 3, **IO)
        set_net(g, 0, net)
        assert (g.progress()[:, 4] != 0).all()
        x = eval_and_record(g, net, path, rng, "finished")
        np.testing.assert_array_equal(x[:, -28], g.winners().reshape(-1).astype(np.float32))
    print("policy_eval ok")


def closed_loop(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    n_envs, cpe = {"5x3": (5, 3), "3x8": (3, 8)}[opt["shape"]]
    nets = [driver_net(21, n_rivals=3, lookahead=4, lookahead_stride=3, out_offset=(2.2, 0.0)), driver_net(22, rivals=False, out_offset=(0.9, 0.0)),
            driver_net(23, n_rivals=7, use_state=False), driver_net(24, n_rivals=1, out_offset=(1.2, 0.0))]
    names = ["net0", "net1", "fast"] if cpe == 3 else ["net0", "net1", "fast", "net2", "net3", "nidc", "net2", "net0"]
    kw = dict(n_envs=n_envs, cars_per_env=cpe, **LOOP)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as o:
        for s, net in enumerate(nets):
            set_net(g, s, net)
        g.set_car_policies(names)
        o.set_car_policies([x if not x.startswith("net") else "lobotomy" for x in names])
        slot = np.array([int(x[3:]) if x.startswith("net") else -1 for x in names] * n_envs)
        of_car = [(nets[s], np.flatnonzero(slot == s)) for s in range(4) if (slot == s).any()]
        rows = []
        for launch in range(3):
            g.rollout("per_car", 50)
            for _ in range(50):
                host_step(o, of_car, path, bundled=True, rows=rows)
            assert_equal_state(read_back(g), read_back(o), f"closed loop, launch {launch}")
        name = g.kernel_name()
        assert name == "ftgp_step_kernel<true, false, true, false, false, true>", name
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
        rows = np.stack(rows)
        assert (rows[:, :, 4 + rm.PRESENT] == 1.0).all(), "mates were present"
        changed = (rows[1:, :, rm.PLACE] != rows[:-1, :, rm.PLACE]).sum()
        assert changed > 0, "no place changed"
        print(f"{opt['shape']}: {int(changed)} place changes")
    print("closed loop ok")


def train_to_deploy(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    L, R = 3, 3
    net = driver_net(41, lookahead=L, n_rivals=R)
    kw = dict(n_envs=7, n_rays=64, cars_per_env=3, action_repeat=1, max_episode_steps=15, scan_pool=net["pool"], scan_max_range=net["max_range"],
              state=True, spawn_mode=1, seed=9, random_start=True, start_lateral=0.6, start_yaw_jitter=0.2, track_frame=True, lookahead=L)
    lo, hi = net["beam_first"], net["beam_first"] + net["n_beams"]
    for what, a_kw in (("the env's rivals as the slot's", dict(rivals=True, n_rivals=R)), ("the env's rivals off", {}), ("n_rivals 1 in the env", dict(n_rivals=1))):
        a = DeviceVecEnv("small-circle", roster=["agent", "net0", "fast"], nets={0: spec_of(net)}, **kw, **a_kw)
        b = DeviceVecEnv("small-circle", roster=["agent", "agent", "fast"], **kw, rivals=True, n_rivals=R)
        assert a.rivals == bool(a_kw) and b.rivals and b.rival.shape == (7, 2, 4 + 8 * R)
        a.reset(); b.reset()
        obs_b, state_b, frame_b, rival_b = b.obs.clone(), b.state.clone(), b.frame.clone(), b.rival.clone()
        resets = 0
        for call in range(40):
            shared = torch.tensor([1.5 + 0.5 * np.sin(0.3 * call), 0.3 * np.cos(0.2 * call)], dtype=torch.float32, device=a.device)
            x = np.concatenate([obs_b[:, 1, lo:hi].cpu().numpy(), state_b[:, 1, :5].cpu().numpy(), frame_b[:, 1].cpu().numpy(), rival_b[:, 1].cpu().numpy()], axis=1)
            assert x.shape[1] == nrm.n_in(net)
            assert (x[:, -8 * R:].reshape(-1, R, 8)[:, :2, rm.PRESENT] == 1).all() and (x[:, -8:] == 0).all()      # two mates, three slots
            u = nm.evaluate(net, None, inputs=x)
            act_a = shared.expand(a.n_envs, 1, 2).contiguous()
            act_b = torch.cat([act_a, torch.from_numpy(u.astype(np.float32)).to(a.device)[:, None, :]], dim=1).contiguous()
            oa, ra, ta, tra, ia = a.step(act_a)
            ob, rb, tb, trb, ib = b.step(act_b)
            where = f"{what}, call {call}"
            assert torch.equal(oa[:, 0], ob[:, 0]) and torch.equal(ra[:, 0], rb[:, 0]) and torch.equal(ia["state"][:, 0], ib["state"][:, 0]), where
            assert torch.equal(ia["frame"][:, 0], ib["frame"][:, 0]), where
            if a_kw.get("rivals"):
                assert torch.equal(ia["rival"][:, 0], ib["rival"][:, 0]), where
            assert torch.equal(ta, tb) and torch.equal(tra, trb), where
            np.testing.assert_array_equal(a.env.pose(), b.env.pose(), err_msg=where)
            np.testing.assert_array_equal(a.env.lidar(), b.env.lidar(), err_msg=where)
            resets += int((ta | tra).sum())
            obs_b, state_b, frame_b, rival_b = ob.clone(), ib["state"].clone(), ib["frame"].clone(), ib["rival"].clone()
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
    nets = [driver_net(51, lookahead=5, lookahead_stride=4, n_rivals=2), driver_net(52, hidden=37, hidden_act="relu", rivals=False)]
    assert nets[0]["frame"] and nets[0]["rivals"] and not nets[1]["frame"] and not nets[1]["rivals"]
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
        # an env on track 1 must use track 1's path for every mate's search: the model with track 0's path for those envs says something else
        on_1 = np.arange(counts[0] * cpe, n * cpe)
        rivals_only = dict(n_rivals=2)
        race = nrm.race_of(g)
        sub = {k: (v[on_1] if k != "cpe" else v) for k, v in race.items()}
        r1 = nrm.rival_block(rivals_only, g.pose()[on_1], sub, [path[c] for c in on_1])
        r0 = nrm.rival_block(rivals_only, g.pose()[on_1], sub, path[0])
        assert not np.array_equal(r0, r1)
        g.rollout("per_car", 30)
        for _ in range(30):
            host_step(twin, of_car, path, bundled=True)
        assert_equal_state(read_back(g), read_back(twin), "multi-track roster with dynamics")
        name = g.kernel_name()
        assert name == "ftgp_step_kernel<true, false, true, true, true, true>", name
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
    print("multitrack ok")


def model_rows(net, env, cars, path, std, noise, lo, hi):
    """(x, mean, action) [n_envs, n_ext, .] of the model for the external cars `cars` on a handle's read-backs: collect_model's decision
    on the wider input vector, which takes the records of every car of the env."""
    n, k = cars.shape
    race = nrm.race_of(env)
    x = nrm.inputs(net, env.lidar(), env.pose(), env.ctrl(), path, race)[cars.reshape(-1)]
    y = nm.forward(x, net["layers"], net["hidden_act"], net["out_act"])
    m = cmod.mean(y, net["out_scale"], net["out_offset"])
    a = cmod.action(m, std, None if noise is None else noise.reshape(n * k, 2), lo, hi)
    fin = (race["finished"] != 0)[cars.reshape(-1)][:, None]
    m, a = np.where(fin, np.float32(0), m).astype(np.float32), np.where(fin, np.float32(0), a).astype(np.float32)
    return x.reshape(n, k, -1), m.reshape(n, k, 2), a.reshape(n, k, 2)


def collect(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    net = driver_net(61, lookahead=3, lookahead_stride=2, n_rivals=3)
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
    buf = Buffers(T, n, k, nrm.n_in(net), next_inputs=True)
    buf.collect(g, T, std=std, clip=clip, noise=nz.data_ptr())
    torch.cuda.synchronize()
    out = buf.host()
    assert out["inputs"].shape[-1] == 12 + 5 + 4 + 6 + 4 + 24
    twin = Twin(tw, roster, 64)
    ended_total = 0
    for s in range(T):
        x, m, a = model_rows(net, tw, cars, path, std, noise[s], lo, hi)
        cmod.assert_same_bits(out["inputs"][s], x, f"inputs[{s}]")
        cmod.assert_same_bits(out["mean"][s], m, f"mean[{s}]")
        cmod.assert_same_bits(out["action"][s], a, f"action[{s}]")
        assert (x[:, :, -28 + 4 + rm.PRESENT] == 1).all() and (x[:, :, -8:] == 0).all()          # two mates in three slots
        reward, term, trunc = twin.step(out["action"][s])
        cmod.assert_same_bits(out["reward"][s], reward, f"reward[{s}]")
        np.testing.assert_array_equal(out["terminated"][s], term, err_msg=f"terminated[{s}]")
        np.testing.assert_array_equal(out["truncated"][s], trunc, err_msg=f"truncated[{s}]")
        ended = (term | trunc).astype(bool)
        ended_total += int(ended.sum())
        after = model_rows(net, tw, cars, path, std, None, lo, hi)[0]          # what the next decision sees
        keep = ~ended
        cmod.assert_same_bits(out["next_inputs"][s][keep], after[keep], f"next_inputs[{s}] without a reset")
        if ended.any():
            assert not cmod.same_bits(out["next_inputs"][s][ended], after[ended]), f"next_inputs[{s}]: the rows before the reset"
    assert ended_total >= n_envs, "no episode ended"
    np.testing.assert_array_equal(records(g), records(tw), err_msg="the env-state records at the end")
    for name, p, q in (("lidar", g.lidar(), tw.lidar()), ("pose", g.pose(), tw.pose()), ("ctrl", g.ctrl(), tw.ctrl()), ("steps", g.steps(), tw.steps())):
        np.testing.assert_array_equal(p, q, err_msg=f"{name} at the end")
    g.close(); tw.close()
    # the rows before a reset, from a twin without auto-reset: next_inputs of the decision that ends an episode
    envs = []
    for auto in (True, False):
        e = capi.Env(lib, t, n_envs=n_envs, cars_per_env=len(roster), n_rays=64, spawn_mode=1, seed=5)
        e.device_io_config(roster, max_episode_steps=6, action_repeat=2, auto_reset=auto)
        envs.append(e)
    g, tw = envs
    set_net(g, 0, net)
    buf = Buffers(3, n, k, nrm.n_in(net), next_inputs=True)
    buf.collect(g, 3, clip=WIDE)
    torch.cuda.synchronize()
    out = buf.host()
    twin = Twin(tw, roster, 64)
    for s in range(3):
        _, term, trunc = twin.step(out["action"][s])
    assert trunc.all() and out["truncated"][2].all()
    before = model_rows(net, tw, cars, path, (0.0, 0.0), None, lo, hi)[0]
    cmod.assert_same_bits(out["next_inputs"][2], before, "next_inputs at a truncation: the records before the reset")
    g.close(); tw.close()
    print("collect ok")


def device_setter(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    shape = dict(lookahead=2, lookahead_stride=9, n_rivals=2)
    net_a, net_b = driver_net(61, **shape), driver_net(62, **shape)
    rng = np.random.default_rng(6)
    kw = dict(n_envs=4, cars_per_env=3, **LOOP)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as h:
        set_net(g, 0, net_a); set_net(h, 0, net_a)
        flat_b = torch.from_numpy(nrm.flat_params(net_b)).to(DEV)
        assert flat_b.numel() == 16 * (25 + 20) + 16 + 2 * 16 + 2
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
        want = model_all(net_b, g, path, scans)[0]
        np.testing.assert_array_equal(g.policy_eval("net0", scans), want)
        # (the larger count was taken: the second layer's parameters lie behind the 16 x 45 of the first)
        host = np.zeros(2000, dtype=np.float32)
        assert g.lib.fn("set_net_device")(g.h, None, 0, host.ctypes.data) == ERR_ARG
        # ftgp_get_net, ftgp_get_net_frame and ftgp_get_net_rivals return what was set: the first layer has the true n_in columns
        for env in (g, h):
            d, layers, extra = env.get_net(0)
            assert (d.pool, d.beam_first, d.n_beams, d.use_state, d.n_layers) == (4, 2, 12, 1, 2) and list(d.width) == [16, 2, 0, 0] and d.reserved == 0
            assert extra == dict(frame=True, lookahead=2, lookahead_stride=9, rivals=True, n_rivals=2), extra
            assert env.net_rivals(0) == dict(rivals=True, n_rivals=2)
            assert layers[0][0].shape == (16, 45)
            for (W, b), (W0, b0) in zip(layers, net_b["layers"]):
                np.testing.assert_array_equal(W, W0); np.testing.assert_array_equal(b, b0)
        # a slot without rival inputs reads zeros
        set_net(g, 1, driver_net(63, rivals=False, lookahead=1))
        assert g.net_rivals(1) == dict(rivals=False, n_rivals=0) and g.net_frame(1)["lookahead"] == 1
        r = capi.FtgpNetRivals(enabled=7, n_rivals=7)
        assert lib.fn("get_net_rivals")(g.h, 1, r) == 0 and (r.enabled, r.n_rivals, tuple(r.reserved)) == (0, 0, (0, 0))
    print("device setter ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    path = np.asarray(t.path, dtype=np.float64)
    rng = np.random.default_rng(4)
    limit = dict(pool=4, max_range=8.0, beam_first=42)
    net = nrm.random_net(rng, (8,), n_beams=155, lookahead=16, n_rivals=7, **limit)                  # n_in = 256
    with capi.Env(lib, t, n_envs=2, cars_per_env=2, n_rays=1344, spawn_mode=1, seed=5) as g:
        r0 = capi.FtgpNetRivals()
        assert lib.fn("get_net_rivals")(g.h, 0, r0) == ERR_STATE and "not defined" in lib.last_error()
        assert lib.fn("get_net_rivals")(g.h, 4, r0) == ERR_ARG and lib.fn("get_net_rivals")(g.h, -1, r0) == ERR_ARG
        scans = nm.eval_scans(rng, g.n_cars, 1344, net["max_range"])
        set_net(g, 0, net)
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        want = model_all(net, g, path, scans)[0]
        d0, flat = capi.net_desc(net["layers"], **nrm.fields(net))
        big = np.zeros(flat.size + 2 * 64, dtype=np.float32)

        def refused(word, expect=ERR_ARG, slot=0, params=flat, desc=None, frame=None, **rivals):
            d = capi.FtgpNetDesc.from_buffer_copy(d0)
            for k, v in (desc or {}).items():
                setattr(d, k, v)
            f = capi.FtgpNetFrame(**{**dict(enabled=1, n_ahead=16, stride=1, reserved=0), **(frame or {})})
            res = rivals.pop("reserved", (0, 0))
            r = capi.FtgpNetRivals(**{**dict(enabled=1, n_rivals=7), **rivals})
            r.reserved[0], r.reserved[1] = res
            rc = lib.fn("set_net_rivals")(g.h, slot, d, f, r, None if params is None else params.ctypes.data)
            assert rc == expect, (rivals, frame, desc, slot, rc, lib.last_error())
            assert word in lib.last_error(), (word, lib.last_error())
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval("net0", scans), want, err_msg=f"slot 0 after {rivals} {frame} {desc}")
            assert g.net_rivals(0) == dict(rivals=True, n_rivals=7) and g.net_frame(0) == dict(frame=True, lookahead=16, lookahead_stride=1)
        refused("enabled", enabled=2); refused("enabled", enabled=-1)
        refused("n_rivals", n_rivals=8); refused("n_rivals", n_rivals=-1)
        refused("n_rivals", enabled=0, n_rivals=8)                                                    # checked with the rivals off too
        refused("reserved", reserved=(1, 0)); refused("reserved", reserved=(0, 1))
        refused("n_in", desc=dict(n_beams=156), params=big)                                           # 156 + 5 + 36 + 60 = 257, reached only through the rival block
        # ftgp_set_net_frame's and ftgp_set_net's own checks, through the new entry
        refused("n_ahead", frame=dict(n_ahead=17)); refused("stride", frame=dict(stride=0)); refused("reserved", frame=dict(reserved=1))
        refused("slot", slot=4); refused("slot", slot=-1); refused("params", params=None)
        refused("pool", desc=dict(pool=5)); refused("reserved", desc=dict(reserved=1)); refused("use_state", desc=dict(use_state=2))
        refused("beam", desc=dict(beam_first=41)); refused("n_layers", desc=dict(n_layers=0))
        # 156 beams without the rival block are fine (n_in = 197), into another slot
        d = capi.FtgpNetDesc.from_buffer_copy(d0); d.n_beams = 156
        f = capi.FtgpNetFrame(enabled=1, n_ahead=16, stride=1)
        assert lib.fn("set_net_rivals")(g.h, 1, d, f, None, big.ctypes.data) == 0, lib.last_error()
        assert lib.fn("set_net_rivals")(g.h, 1, d, f, capi.FtgpNetRivals(enabled=0, n_rivals=7), big.ctypes.data) == 0, lib.last_error()
        assert g.net_rivals(1) == dict(rivals=False, n_rivals=0) and g.net_frame(1)["lookahead"] == 16
    # enabled == 0 and rivals == NULL are ftgp_set_net_frame to the letter
    small = driver_net(81, rivals=False, lookahead=2)
    with capi.Env(lib, t, n_envs=2, cars_per_env=2, **LOOP) as g:
        scans = nm.eval_scans(rng, g.n_cars, 64, small["max_range"])
        d0, flat = capi.net_desc(small["layers"], **nrm.fields(small))
        f = capi.FtgpNetFrame(enabled=1, n_ahead=2, stride=1)
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        want = model_all(small, g, path, scans)[0]
        assert lib.fn("set_net_frame")(g.h, 0, d0, f, flat.ctypes.data) == 0
        assert lib.fn("set_net_rivals")(g.h, 1, d0, f, None, flat.ctypes.data) == 0
        assert lib.fn("set_net_rivals")(g.h, 2, d0, f, capi.FtgpNetRivals(enabled=0, n_rivals=5), flat.ctypes.data) == 0
        for s in range(3):
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval(f"net{s}", scans), want, err_msg=f"slot {s}")
            assert g.net(s)[1][0][0].shape == (16, 25)
    with capi.Env(lib, t, n_envs=1, n_rays=64, lidar_mode="fakelidar") as f:
        assert lib.fn("set_net_rivals")(f.h, 0, d0, None, capi.FtgpNetRivals(enabled=1, n_rivals=0), flat.ctypes.data) == ERR_STATE
    print("errors ok")


def no_rival_slot(opt):
    lib = capi.load()
    t = load_track("small-circle")
    kw = dict(n_envs=4, cars_per_env=3, **LOOP)
    plain = driver_net(71, rivals=False)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as fresh, capi.Env(lib, t, **kw) as twin:
        set_net(g, 0, plain); set_net(g, 1, driver_net(72, n_rivals=3))
        set_net(fresh, 0, plain)
        for e in (g, fresh):
            e.rollout("fast", 30)
        assert g.kernel_name() == fresh.kernel_name() == "ftgp_step_kernel<true, false, false>", (g.kernel_name(), fresh.kernel_name())
        for e in (g, fresh):
            e.rollout("net0", 30)
        net_name = fresh.kernel_name()
        assert g.kernel_name() == net_name and is_net_kernel(net_name), (g.kernel_name(), net_name)
        assert_equal_state(read_back(g), read_back(fresh), "rollout net0 beside a slot with rival inputs")
        # ... and the same bits as the model of the network without rival inputs gives through the host
        twin.rollout("fast", 30)
        path = np.asarray(t.path, dtype=np.float64)
        for _ in range(30):
            host_step(twin, [(plain, np.arange(twin.n_cars))], path)
        assert_equal_state(read_back(g), read_back(twin), "rollout net0 against the host")
        for e in (g, fresh):
            e.set_car_policies(["net0", "fast", "lobotomy"])
            e.rollout("per_car", 30)
        assert g.kernel_name() == fresh.kernel_name() and is_net_kernel(g.kernel_name()), (g.kernel_name(), fresh.kernel_name())
        assert_equal_state(read_back(g), read_back(fresh), "a roster with a slot without rival inputs")
        g.rollout("net1", 5)
        assert g.kernel_name() == net_name, g.kernel_name()                # a rival slot has no kernels of its own
    print("no rival slot ok")


SCENARIOS = {"policy_eval": policy_eval, "closed_loop": closed_loop, "train_to_deploy": train_to_deploy, "multitrack": multitrack,
             "collect": collect, "device_setter": device_setter, "errors": errors, "no_rival_slot": no_rival_slot}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
