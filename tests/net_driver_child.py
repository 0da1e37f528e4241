"""Child process of tests/test_net_driver.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/net_driver_child.py <scenario> [json options]

The criterion throughout: what the library computes with a network driver equals, bit for bit, what the numpy model of the header's
text (tests/net_model.py) computes from the same scans and records -- evaluated on the host and fed back as host controls to a twin
that knows nothing of networks.
"""
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
from tests import helpers  # noqa: E402
from tests import net_model as nm  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
LOOP = dict(n_rays=64, spawn_mode=1, seed=5)
# a driver for 64 rays: beams 2 .. 13 of pool 4 and the state, speed in [0.5, 2.5], steering in [-0.5, 0.5]
DRIVER = dict(pool=4, max_range=3.0, beam_first=2, use_state=True, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))


def fields(net):
    return {k: v for k, v in net.items() if k != "layers"}


def set_net(env, slot, net):
    env.set_net(slot, net["layers"], **fields(net))


def driver_net(seed, hidden=16, **over):
    return nm.random_net(np.random.default_rng(seed), (17, hidden, 2), **{**DRIVER, **over})


def read_back(g):
    return dict(lidar=g.lidar(), pose=g.pose(), progress=g.progress(), ctrl=g.ctrl(), steps=g.steps())


def assert_equal_state(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def host_step(twin, nets_of_car, bundled=None):
    """One step of a twin through the host: every car's controls from the model of its network on lidar() + pose() + get_ctrl() --
    or, for a car without one, from policy_eval of its bundled driver -- then set_ctrl and step(1)."""
    scans, pose, ctrl = twin.lidar(), twin.pose(), twin.ctrl()
    finished = twin.progress()[:, 4] != 0
    u = twin.policy_eval("per_car", scans) if bundled else np.zeros((twin.n_cars, 2))
    for net, cars in nets_of_car:
        u[cars] = nm.evaluate(net, scans[cars], pose[cars], ctrl[cars], finished[cars])
    twin.set_ctrl(u)
    twin.step(1)


def is_net_kernel(name):
    return name.count(",") == 5 and name.endswith("true>")


def policy_eval(opt):
    lib = capi.load()
    rng = np.random.default_rng(3)
    for name, (n_rays, nets) in nm.eval_cases().items():
        t = load_track("small-circle")
        with capi.Env(lib, t, n_envs=3, cars_per_env=2, n_rays=n_rays, spawn_mode=1, seed=2) as g:
            for s, net in enumerate(nets):
                set_net(g, s, net)
            pose, ctrl = nm.eval_records(rng, g.n_cars)
            pose[:, :3] = g.pose()[:, :3]
            for s, net in enumerate(nets):
                scans = nm.eval_scans(rng, g.n_cars, n_rays, net["max_range"])
                g.set_pose(pose); g.set_ctrl(ctrl)
                got = g.policy_eval(f"net{s}", scans)
                want = nm.evaluate(net, scans, g.pose(), ctrl)
                np.testing.assert_array_equal(got, want, err_msg=f"{name}, slot {s}")
                np.testing.assert_array_equal(g.ctrl(), want, err_msg=f"{name}, slot {s}: stored controls")
                assert np.abs(want).max() > 0, name
            # an infinite weight: the guard gives (0, 0)
            bad = dict(nets[0], out_act="identity", layers=[(W.copy(), b.copy()) for W, b in nets[0]["layers"]])
            bad["layers"][-1][0][1, 0] = np.inf                  # (in front of an identity output: the sum is infinite or a NaN)
            set_net(g, 0, bad)
            scans = nm.eval_scans(rng, g.n_cars, n_rays, bad["max_range"])
            g.set_ctrl(ctrl)
            got = g.policy_eval("net0", scans)
            np.testing.assert_array_equal(got, 0.0, err_msg=f"{name}: infinite weight")
            np.testing.assert_array_equal(nm.evaluate(bad, scans, g.pose(), ctrl), 0.0)
        print(f"policy_eval {name} ok")
    # finished cars get (0, 0) before the network is looked at
    n_rays, nets = nm.eval_cases()["one_layer"]
    with capi.Env(lib, load_track("small-circle"), n_envs=2, n_rays=n_rays, lap_target=0) as g:
        assert g.progress()[:, 4].all()
        set_net(g, 0, nets[0])
        scans = nm.eval_scans(rng, g.n_cars, n_rays, nets[0]["max_range"])
        assert np.abs(nm.evaluate(nets[0], scans, g.pose(), g.ctrl())).max() > 0
        np.testing.assert_array_equal(g.policy_eval("net0", scans), 0.0)
    print("policy_eval ok")


def closed_loop(opt):
    lib, ora = helpers.libs()
    t = load_track("small-circle")
    net = driver_net(21)
    with capi.Env(lib, t, n_envs=19, **LOOP) as g, capi.Env(ora, t, n_envs=19, **LOOP) as o:
        set_net(g, 0, net)
        everyone = [(net, np.arange(o.n_cars))]
        for launch in range(3):
            g.rollout("net0", 50)
            for _ in range(50):
                host_step(o, everyone)
            assert_equal_state(read_back(g), read_back(o), f"closed loop, launch {launch}")
        assert is_net_kernel(g.kernel_name()), g.kernel_name()
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
    print("closed loop ok")


def roster(opt):
    lib = capi.load()
    t = load_track("small-circle")
    nets = [driver_net(31), driver_net(32, hidden=37, hidden_act="relu")]
    for names, wrap in ((["net0", "nidc", "net1"], False), (["net0", "fast", "net1", "nidc", "net0", "lobotomy"], True)):
        cpe = len(names)
        kw = dict(n_envs=3, cars_per_env=cpe, bubble_wrap=wrap, **LOOP)
        with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as twin:
            for s, net in enumerate(nets):
                set_net(g, s, net)
            g.set_car_policies(names)
            twin.set_car_policies([n if not n.startswith("net") else "lobotomy" for n in names])
            slot = np.array([int(n[3:]) if n.startswith("net") else -1 for n in names] * g.n_envs)
            of_car = [(nets[s], np.flatnonzero(slot == s)) for s in range(2)]
            g.rollout("per_car", 40)
            for _ in range(40):
                host_step(twin, of_car, bundled=True)
            assert_equal_state(read_back(g), read_back(twin), f"roster {names}")
            assert is_net_kernel(g.kernel_name()) and not is_net_kernel(twin.kernel_name()), (g.kernel_name(), twin.kernel_name())
        print(f"roster {cpe} ok")
    print("roster ok")


def device_step(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    net = driver_net(41)
    kw = dict(n_envs=7, n_rays=64, cars_per_env=2, action_repeat=1, max_episode_steps=15, scan_pool=net["pool"], scan_max_range=net["max_range"],
              state=True, spawn_mode=1, seed=9)
    a = DeviceVecEnv("small-circle", roster=["agent", "net0"], nets={0: nm_spec(net)}, **kw)
    b = DeviceVecEnv("small-circle", roster=["agent", "agent"], **kw)
    lo, hi = net["beam_first"], net["beam_first"] + net["n_beams"]
    a.reset(); b.reset()
    obs_b, state_b = b.obs.clone(), b.state.clone()
    resets = 0
    for call in range(40):
        shared = torch.tensor([1.5 + 0.5 * np.sin(0.3 * call), 0.3 * np.cos(0.2 * call)], dtype=torch.float32, device=a.device)
        x = np.concatenate([obs_b[:, 1, lo:hi].cpu().numpy(), state_b[:, 1, :5].cpu().numpy()], axis=1)
        u = nm.evaluate(net, None, inputs=x)
        act_a = shared.expand(a.n_envs, 1, 2).contiguous()
        act_b = torch.cat([act_a, torch.from_numpy(u.astype(np.float32)).to(a.device)[:, None, :]], dim=1).contiguous()
        oa, ra, ta, tra, ia = a.step(act_a)
        ob, rb, tb, trb, ib = b.step(act_b)
        what = f"device step, call {call}"
        assert torch.equal(oa[:, 0], ob[:, 0]) and torch.equal(ra[:, 0], rb[:, 0]) and torch.equal(ia["state"][:, 0], ib["state"][:, 0]), what
        assert torch.equal(ta, tb) and torch.equal(tra, trb), what
        np.testing.assert_array_equal(a.env.pose(), b.env.pose(), err_msg=what)
        resets += int((ta | tra).sum())
        obs_b, state_b = ob.clone(), ib["state"].clone()
    assert resets >= 7, "no auto-reset happened"
    assert is_net_kernel(a.env.kernel_name()), a.env.kernel_name()
    a.close(); b.close()
    print("device step ok")


def nm_spec(net):
    from ft_grandprix_amd.net import NetSpec
    return NetSpec(net["layers"], **fields(net))


def multitrack(opt):
    lib = capi.load()
    tracks = [load_track("small-circle"), load_track("circle")]
    counts = (5, 6)
    n = sum(counts)
    net = driver_net(51)
    with capi.Env(lib, tracks, n_envs=n, envs_per_track=counts, **LOOP) as g, capi.Env(lib, tracks, n_envs=n, envs_per_track=counts, **LOOP) as twin:
        rows = g.base_dynamics() * np.random.default_rng(8).uniform(helpers.DYN_LO, helpers.DYN_HI, (n, 8))
        for e in (g, twin):
            e.set_dynamics(rows.reshape(n, 1, 8))
        set_net(g, 0, net)
        g.rollout("net0", 30)
        for _ in range(30):
            host_step(twin, [(net, np.arange(n))])
        assert_equal_state(read_back(g), read_back(twin), "multi-track with dynamics")
        name = g.kernel_name()
        assert name == "ftgp_step_kernel<false, false, true, true, true, true>", name
    print("multitrack ok")


def device_setter(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net_a, net_b = driver_net(61), driver_net(62)
    rng = np.random.default_rng(6)
    with capi.Env(lib, t, n_envs=5, **LOOP) as g, capi.Env(lib, t, n_envs=5, **LOOP) as h:
        set_net(g, 0, net_a); set_net(h, 0, net_a)
        flat_b = torch.from_numpy(np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in net_b["layers"]])).to("cuda")
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
        # the controls the host setter gives
        scans = nm.eval_scans(rng, g.n_cars, 64, net_b["max_range"])
        ctrl = g.ctrl()
        want = nm.evaluate(net_b, scans, g.pose(), ctrl)
        np.testing.assert_array_equal(g.policy_eval("net0", scans), want)
        # ftgp_get_net returns what was set
        for env in (g, h):
            d, layers = env.net(0)
            assert (d.pool, d.beam_first, d.n_beams, d.use_state, d.n_layers, d.hidden_act, d.out_act) == (4, 2, 12, 1, 2, capi.ACT_TANH, capi.ACT_TANH)
            assert list(d.width) == [16, 2, 0, 0] and d.max_range == np.float32(3.0) and list(d.out_scale) == [1.0, 0.5] and list(d.out_offset) == [1.5, 0.0]
            for (W, b), (W0, b0) in zip(layers, net_b["layers"]):
                np.testing.assert_array_equal(W, W0); np.testing.assert_array_equal(b, b0)
        # a host pointer is refused before anything is enqueued; an undefined slot is a state error
        host = np.zeros(1000, dtype=np.float32)
        assert g.lib.fn("set_net_device")(g.h, None, 0, host.ctypes.data) == ERR_ARG and "ftgp_set_net_device" in g.lib.last_error()
        assert g.lib.fn("set_net_device")(g.h, None, 1, flat_b.data_ptr()) == ERR_STATE
        g.set_ctrl(ctrl)                                         # (the state inputs: policy_eval stored its controls)
        np.testing.assert_array_equal(g.policy_eval("net0", scans), want)
    print("device setter ok")


def no_network(opt):
    lib = capi.load()
    t = load_track("small-circle")
    kw = dict(n_envs=4, cars_per_env=3, **LOOP)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as fresh:
        set_net(g, 0, driver_net(71))
        for e in (g, fresh):
            e.rollout("fast", 50)
        assert g.kernel_name() == fresh.kernel_name() == "ftgp_step_kernel<true, false, false>", (g.kernel_name(), fresh.kernel_name())
        assert_equal_state(read_back(g), read_back(fresh), "rollout fast beside a defined slot")
        for e in (g, fresh):
            e.set_car_policies(["nidc", "fast", "lobotomy"])
            e.rollout("per_car", 50)
        assert g.kernel_name() == fresh.kernel_name() == "ftgp_step_kernel<true, false, true>", (g.kernel_name(), fresh.kernel_name())
        assert_equal_state(read_back(g), read_back(fresh), "rollout per_car of bundled drivers beside a defined slot")
        # reset leaves the networks alone
        g.reset()
        g.rollout("net0", 5)
        assert is_net_kernel(g.kernel_name())
    print("no network ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = driver_net(81)
    rng = np.random.default_rng(4)
    with capi.Env(lib, t, n_envs=2, cars_per_env=2, **LOOP) as g:
        scans = nm.eval_scans(rng, g.n_cars, 64, net["max_range"])

        def code(call, *a, **k):
            try:
                call(*a, **k)
            except capi.FtgpError as x:
                return x.code
            return 0
        # an undefined slot: at the call that would launch it
        assert code(g.rollout, "net0", 1) == ERR_STATE and code(g.policy_eval, "net2", scans) == ERR_STATE
        g.set_car_policies(["net1", "fast"])
        assert code(g.rollout, "per_car", 1) == ERR_STATE and code(g.policy_eval, "per_car", scans) == ERR_STATE
        g.device_io_config(["agent", "net3"])
        z = torch.zeros(4096, dtype=torch.float32, device="cuda")
        assert code(g.step_device, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr()) == ERR_STATE
        assert code(g.rollout, 10, 1) == ERR_ARG and code(g.set_car_policies, ["net0", 10]) == ERR_ARG
        set_net(g, 0, net)
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        want = nm.evaluate(net, scans, g.pose(), g.ctrl())
        d0, flat = capi.net_desc(net["layers"], **fields(net))

        def refused(expect=ERR_ARG, slot=0, params=flat, **change):
            d = capi.FtgpNetDesc.from_buffer_copy(d0)
            for k, v in change.items():
                if isinstance(v, tuple):
                    getattr(d, k)[v[0]] = v[1]
                else:
                    setattr(d, k, v)
            rc = lib.fn("set_net")(g.h, slot, d, None if params is None else params.ctypes.data)
            assert rc == expect, (change, slot, rc, lib.last_error())
            if change:
                assert next(iter(change)).split("_")[0] in lib.last_error() or "beam" in lib.last_error(), (change, lib.last_error())
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval("net0", scans), want, err_msg=f"slot 0 after {change}")
        refused(slot=-1); refused(slot=4); refused(params=None)
        refused(pool=3); refused(pool=0); refused(max_range=0.0); refused(max_range=float("inf")); refused(max_range=float("nan"))
        refused(beam_first=1); refused(n_beams=13); refused(n_beams=0); refused(beam_first=-1)
        refused(use_state=2); refused(n_layers=0); refused(n_layers=5)
        refused(width=(0, 0)); refused(width=(0, 129)); refused(width=(1, 3)); refused(width=(2, 1))
        refused(hidden_act=3); refused(out_act=-1)
        refused(out_scale=(0, float("inf"))); refused(out_offset=(1, float("nan"))); refused(reserved=1)
    with capi.Env(lib, t, n_envs=1, n_rays=64, lidar_mode="fakelidar") as f:
        d0, flat = capi.net_desc(net["layers"], **fields(net))
        assert lib.fn("set_net")(f.h, 0, d0, flat.ctypes.data) == ERR_STATE
    print("errors ok")


SCENARIOS = {"policy_eval": policy_eval, "closed_loop": closed_loop, "roster": roster, "device_step": device_step, "multitrack": multitrack,
             "device_setter": device_setter, "no_network": no_network, "errors": errors}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
