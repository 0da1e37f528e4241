"""Child process of tests/test_collect.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/collect_child.py <scenario> [json options]

The criterion throughout (include/ftgp.h "Collected rollouts", the contract): after ftgp_collect_device the handle and the outputs are,
to the bit, what T calls of ftgp_step_device_rivals fed action[0 .. T-1] leave on a twin handle; and inputs, mean and action of
decision t are what the numpy model of the header's text (tests/collect_model.py, tests/net_model.py) computes from the twin's
read-backs before its call t.  No tolerance anywhere.
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
from tests import collect_model as cmod  # noqa: E402
from tests import net_model as nm  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
DEV = "cuda"
# a driver for 64 rays: beams 2 .. 13 of pool 4 and the state, speed in [0.5, 2.5], steering in [-0.5, 0.5]
DRIVER = dict(pool=4, max_range=3.0, beam_first=2, use_state=True, out_scale=(1.0, 0.5), out_offset=(1.5, 0.0))
WIDE = ((-1e30, 1e30), (-1e30, 1e30))


def fields(net):
    return {k: v for k, v in net.items() if k != "layers"}


def set_net(env, slot, net):
    env.set_net(slot, net["layers"], **fields(net))


def driver_net(seed, hidden=16, **over):
    return nm.random_net(np.random.default_rng(seed), (17, hidden, 2), **{**DRIVER, **over})


def zeros(shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def ext_cars(env, roster):
    """The car index of external car i of env e, [n_envs, n_ext]."""
    slots = np.array([k for k, r in enumerate(roster) if r == "agent"])
    return np.arange(env.n_envs)[:, None] * env.cars_per_env + slots[None, :]


def records(env):
    """The ftgp_save_envs_device records of every env, as bytes on the host."""
    rows = zeros((env.n_envs, env.env_state_bytes()), torch.uint8)
    env.save_envs_device(rows.data_ptr(), env.n_envs)
    return rows.cpu().numpy()


class Buffers:
    """The buffers of one ftgp_collect_device call (torch tensors on the device)."""

    def __init__(self, T, n_envs, n_ext, n_in, next_inputs=False):
        lead = (T, n_envs, n_ext)
        self.inputs, self.mean, self.action = zeros(lead + (n_in,)), zeros(lead + (2,)), zeros(lead + (2,))
        self.reward, self.terminated, self.truncated = zeros(lead), zeros((T, n_envs), torch.uint8), zeros((T, n_envs), torch.uint8)
        self.next_inputs = zeros(lead + (n_in,)) if next_inputs else None

    def collect(self, env, T, **kw):
        env.collect_device(T, self.inputs.data_ptr(), self.mean.data_ptr(), self.action.data_ptr(), self.reward.data_ptr(),
                           self.terminated.data_ptr(), self.truncated.data_ptr(),
                           next_inputs=0 if self.next_inputs is None else self.next_inputs.data_ptr(), **kw)

    def host(self):
        return {k: v.cpu().numpy() for k, v in vars(self).items() if v is not None}


class Twin:
    """A second handle stepped one ftgp_step_device_rivals call at a time, with the read-backs the model needs before each."""

    def __init__(self, env, roster, n_beams, state=False):
        self.env, self.cars = env, ext_cars(env, roster)
        n, k = self.cars.shape
        self.obs, self.final_obs = zeros((n, k, n_beams)), zeros((n, k, n_beams))
        self.reward, self.terminated, self.truncated = zeros((n, k)), zeros(n, torch.uint8), zeros(n, torch.uint8)
        self.state = zeros((n, k, capi.STATE_FLOATS)) if state else None
        self.final_state = zeros((n, k, capi.STATE_FLOATS)) if state else None

    def read(self):
        e, c = self.env, self.cars
        return dict(scans=e.lidar()[c], pose=e.pose()[c], ctrl=e.ctrl()[c], finished=e.progress()[c, 4] != 0)

    def step(self, action):
        a = torch.from_numpy(np.ascontiguousarray(action, dtype=np.float32)).to(DEV)
        self.env.step_device_rivals(a.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                    self.truncated.data_ptr(), self.final_obs.data_ptr(),
                                    state=0 if self.state is None else self.state.data_ptr(),
                                    final_state=0 if self.final_state is None else self.final_state.data_ptr())
        torch.cuda.synchronize()
        return self.reward.cpu().numpy(), self.terminated.cpu().numpy(), self.truncated.cpu().numpy()


def model_rows(net, rb, std, noise, lo, hi):
    """(x, mean, action) [n_envs, n_ext, .] of the model on a twin's read-backs."""
    n, k = rb["finished"].shape
    flat = lambda a: a.reshape((n * k,) + a.shape[2:])          # noqa: E731
    x, m, a = cmod.act(net, flat(rb["scans"]), flat(rb["pose"]), flat(rb["ctrl"]), flat(rb["finished"]), std, None if noise is None else flat(noise), lo, hi)
    return x.reshape(n, k, -1), m.reshape(n, k, 2), a.reshape(n, k, 2)


def replay(what, g, twin_env, roster, net, T, *, std=(0.0, 0.0), clip=WIDE, noise=None, n_beams=None, dyn_rows=None, slot=0):
    """Collect T decisions on g, replay them on the twin, compare everything; returns the host copies and counters."""
    cars = ext_cars(g, roster)
    n, k = cars.shape
    n_in = net["n_beams"] + (5 if net.get("use_state") else 0)
    buf = Buffers(T, n, k, n_in)
    nz = None if noise is None else torch.from_numpy(noise).to(DEV)
    rows = None if dyn_rows is None else torch.from_numpy(dyn_rows).to(DEV)
    buf.collect(g, T, slot=slot, std=std, clip=clip, noise=0 if nz is None else nz.data_ptr(), reset_dynamics=0 if rows is None else rows.data_ptr())
    torch.cuda.synchronize()
    out = buf.host()
    lo, hi = (clip[0][0], clip[1][0]), (clip[0][1], clip[1][1])
    twin = Twin(twin_env, roster, n_beams or g.n_rays)
    count = dict(ended=0, terminated=0, bound=0, free=0, finished_rows=0)
    for t in range(T):
        rb = twin.read()
        x, m, a = model_rows(net, rb, std, None if noise is None else noise[t], lo, hi)
        cmod.assert_same_bits(out["inputs"][t], x, f"{what}: inputs[{t}]")
        cmod.assert_same_bits(out["mean"][t], m, f"{what}: mean[{t}]")
        cmod.assert_same_bits(out["action"][t], a, f"{what}: action[{t}]")
        reward, term, trunc = twin.step(out["action"][t])
        cmod.assert_same_bits(out["reward"][t], reward, f"{what}: reward[{t}]")
        np.testing.assert_array_equal(out["terminated"][t], term, err_msg=f"{what}: terminated[{t}]")
        np.testing.assert_array_equal(out["truncated"][t], trunc, err_msg=f"{what}: truncated[{t}]")
        if rows is not None:
            mask = torch.from_numpy((term | trunc).astype(np.uint8)).to(DEV)
            twin_env.set_dynamics_device(rows[t].data_ptr(), mask.data_ptr())
            torch.cuda.synchronize()
        live = ~rb["finished"]
        at_bound = ((a == np.float32(lo)) | (a == np.float32(hi))).any(axis=2)
        count["bound"] += int((at_bound & live).sum()); count["free"] += int((~at_bound & live).sum())
        count["ended"] += int((term | trunc).sum()); count["terminated"] += int(term.sum()); count["finished_rows"] += int((~live).sum())
    np.testing.assert_array_equal(records(g), records(twin_env), err_msg=f"{what}: the env-state records at the end")
    np.testing.assert_array_equal(g.episodes(), twin_env.episodes(), err_msg=f"{what}: episodes")
    for name, a, b in (("lidar", g.lidar(), twin_env.lidar()), ("pose", g.pose(), twin_env.pose()), ("ctrl", g.ctrl(), twin_env.ctrl()),
                       ("progress", g.progress(), twin_env.progress()), ("steps", g.steps(), twin_env.steps())):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name} at the end")
    print(f"{what}: {count}")
    return out, count


def pair(lib, track, roster, net, n_envs, n_rays, io, setup=None, **kw):
    """Two handles configured alike, the network in slot 0 of the first (the twin needs none: it is fed actions)."""
    envs = []
    for _ in range(2):
        e = capi.Env(lib, track, n_envs=n_envs, cars_per_env=len(roster), n_rays=n_rays, spawn_mode=1, seed=5, **kw)
        e.device_io_config(roster, **io)
        if setup:
            setup(e)
        envs.append(e)
    set_net(envs[0], 0, net)
    return envs


def replay_and_model(opt):
    lib = capi.load()
    t = load_track("small-circle")
    T = 12
    io = dict(max_episode_steps=5, action_repeat=1, auto_reset=True)
    cases = nm.eval_cases()
    shapes = (("one_layer 7x1", ["agent"], 7, 64, cases["one_layer"][1][0], (0.4, 0.3), ((0.2, 1.0), (-1.5, -0.5))),
              ("mlp_tanh 3x3", ["agent", "fast", "agent"], 3, 1080, cases["mlp_tanh"][1][0], (1.0, 0.3), ((0.5, 4.5), (-0.3, 0.3))),
              ("off_wave 3x3", ["agent", "fast", "agent"], 3, 1080, cases["off_wave"][1][2], (0.5, 0.5), ((0.0, 0.8), (-0.5, 0.5))))
    for what, roster, n_envs, n_rays, net, std, clip in shapes:
        g, twin = pair(lib, t, roster, net, n_envs, n_rays, io)
        n_ext = roster.count("agent")
        assert (n_envs * n_ext) % 4 != 0
        noise = np.random.default_rng(7).standard_normal((T, n_envs, n_ext, 2)).astype(np.float32)
        out, count = replay(what, g, twin, roster, net, T, std=std, clip=clip, noise=noise)
        ended = (out["terminated"] | out["truncated"]).astype(bool)
        assert ended[4].all() and ended[9].all() and ended.sum() == 2 * n_envs, f"{what}: every env ends at its fifth and tenth decision"
        assert out["truncated"][4].all() and not out["terminated"].any()
        assert count["bound"] > 0 and count["free"] > 0, f"{what}: the clip binds for some rows only: {count}"
        assert (out["inputs"][5][..., :net["n_beams"]] == 0).all(), f"{what}: the beams right after a reset are zeros"
        assert np.abs(out["inputs"][4][..., :net["n_beams"]]).max() > 0
        g.close(); twin.close()
    print("replay and model ok")


def offset_steps(envs, mask):
    """Two idle steps for everyone, then a reset of the envs of `mask`: the others are two steps into their episode."""
    for e in envs:
        e.rollout("lobotomy", 2)
        e.reset(np.asarray(mask, dtype=np.uint8))


def next_inputs(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = nm.eval_cases()["mlp_tanh"][1][1]
    roster, n_envs, T = ["agent", "agent"], 3, 9
    io = dict(max_episode_steps=4, action_repeat=1, auto_reset=True)
    g, tw = pair(lib, t, roster, net, n_envs, 1080, io, setup=lambda e: e.device_io_signals(net["pool"], net["max_range"]))
    offset_steps((g, tw), [1, 0, 1])                 # env 1 ends two decisions before the others
    n_in, lo_b, hi_b = 85, net["beam_first"], net["beam_first"] + net["n_beams"]
    buf = Buffers(T, n_envs, 2, n_in, next_inputs=True)
    noise = torch.from_numpy(np.random.default_rng(9).standard_normal((T, n_envs, 2, 2)).astype(np.float32)).to(DEV)
    buf.collect(g, T, std=(0.5, 0.2), clip=((0.0, 5.0), (-0.5, 0.5)), noise=noise.data_ptr())
    torch.cuda.synchronize()
    out = buf.host()
    twin = Twin(tw, roster, 1080 // net["pool"], state=True)
    resets = 0
    for t_ in range(T):
        _, term, trunc = twin.step(out["action"][t_])
        ended = (term | trunc).astype(bool)
        resets += int(ended.sum())
        obs, state = twin.obs.cpu().numpy(), twin.state.cpu().numpy()
        fobs, fstate = twin.final_obs.cpu().numpy(), twin.final_state.cpu().numpy()
        after = np.concatenate([obs[:, :, lo_b:hi_b], state[:, :, :5]], axis=2)              # what the next decision sees
        before_reset = np.concatenate([fobs[:, :, lo_b:hi_b], fstate[:, :, :5]], axis=2)
        want = np.where(ended[:, None, None], before_reset, after)
        cmod.assert_same_bits(out["next_inputs"][t_], want, f"next_inputs[{t_}]")
        if t_ + 1 < T:
            cmod.assert_same_bits(out["inputs"][t_ + 1], after, f"inputs[{t_ + 1}] against the twin's obs and state")
            keep = ~ended
            cmod.assert_same_bits(out["next_inputs"][t_][keep], out["inputs"][t_ + 1][keep], f"next_inputs[{t_}] == inputs[{t_ + 1}] without a reset")
            if ended.any():
                assert (out["inputs"][t_ + 1][ended][..., :net["n_beams"]] == 0).all(), "zero beams after a reset"
                assert (out["inputs"][t_ + 1][ended][..., -2:] == 0).all(), "the spawn state has no controls"
                assert np.abs(out["next_inputs"][t_][ended][..., :net["n_beams"]]).max() > 0
                assert not cmod.same_bits(out["next_inputs"][t_][ended], out["inputs"][t_ + 1][ended])
    assert resets >= 4, resets
    np.testing.assert_array_equal(records(g), records(tw))
    g.close(); tw.close()
    print("next inputs ok")


def against_roster(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = driver_net(21)
    T = 20
    kw = dict(n_envs=5, n_rays=64, spawn_mode=1, seed=5)
    with capi.Env(lib, t, **kw) as g, capi.Env(lib, t, **kw) as r:
        set_net(g, 0, net); set_net(r, 0, net)
        g.device_io_config(["agent"], max_episode_steps=0, action_repeat=1, auto_reset=True)
        buf = Buffers(T, 5, 1, 17)
        buf.collect(g, T, clip=WIDE)
        torch.cuda.synchronize()
        r.rollout("net0", T)
        np.testing.assert_array_equal(g.pose(), r.pose(), err_msg="pose against ftgp_rollout(net0)")
        np.testing.assert_array_equal(g.lidar(), r.lidar(), err_msg="lidar against ftgp_rollout(net0)")
        out = buf.host()
        assert not out["terminated"].any() and not out["truncated"].any()
        assert np.abs(g.pose()[:, 7:9]).max() > 0.1, "the cars did not move"
        cmod.assert_same_bits(out["action"], out["mean"], "no noise, a wide clip: action = mean")
    print("against roster ok")


def rules(opt):
    lib = capi.load()
    small, circle = load_track("small-circle"), load_track("circle")
    fast_net = driver_net(33, out_scale=(1.0, 0.3), out_offset=(4.0, 0.0))      # fast and nearly straight: it meets the wall
    net = driver_net(34)
    T = 12
    noise = lambda n, k: np.random.default_rng(3).standard_normal((T, n, k, 2)).astype(np.float32)      # noqa: E731
    scen = opt.get("only")

    def run(what, track, roster, the_net, n_envs, io, setup=None, clip=((0.0, 6.0), (-0.5, 0.5)), **kw):
        if scen and scen != what:
            return None
        g, tw = pair(lib, track, roster, the_net, n_envs, 64, io, setup=setup, **kw)
        out, count = replay(what, g, tw, roster, the_net, T, std=(0.3, 0.2), clip=clip, noise=noise(n_envs, roster.count("agent")))
        g.close(); tw.close()
        return out, count

    r = run("contacts", small, ["agent", "agent"], fast_net, 5, dict(max_episode_steps=0, action_repeat=25, auto_reset=True),
            setup=lambda e: e.device_io_contacts(True, terminate_on_wall=True, terminate_on_car=True, wall_penalty=2.0, car_penalty=1.0))
    if r:
        assert r[1]["terminated"] > 0, f"no contact ended an env: {r[1]}"
    r = run("dense progress", small, ["agent", "nidc"], net, 5, dict(max_episode_steps=7, action_repeat=4, auto_reset=True),
            setup=lambda e: e.device_io_frame(True, n_ahead=2, stride=3, dense_progress=True))
    if r:
        rew = r[0]["reward"]
        assert np.any(rew != np.round(rew)), "a dense reward is no integer"
    r = run("spawn rule", small, ["agent", "agent"], net, 5, dict(max_episode_steps=4, action_repeat=2, auto_reset=True),
            setup=lambda e: e.set_spawn_rule(True, margin=e.cfg.vehicle.contact_radius, lateral_frac=0.5, yaw_tan=0.1, shuffle_grid=True))
    if r:
        assert r[1]["ended"] == 30         # 2 steps a decision: every env ends at every second decision
    r = run("two tracks", [small, circle], ["agent"], net, 5, dict(max_episode_steps=5, action_repeat=2, auto_reset=True), envs_per_track=(2, 3))
    r = run("action repeat 3", small, ["agent", "fast", "agent"], net, 3, dict(max_episode_steps=9, action_repeat=3, auto_reset=True))
    if r:
        assert r[1]["ended"] == 12         # 3 steps a decision: every env ends at its third, sixth, ninth and twelfth decision
    r = run("place reward", small, ["agent", "agent", "nidc"], net, 3, dict(max_episode_steps=0, action_repeat=5, auto_reset=True),
            setup=lambda e: e.device_io_rivals(True, n_rivals=2, place_weight=0.5))
    print("rules ok" if not scen else f"rules {scen} ok")


def finished_and_diverged(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = driver_net(41)
    roster, T = ["agent", "agent"], 4
    io = dict(max_episode_steps=0, action_repeat=1, auto_reset=False)
    # lap_target 0: every car has finished from the start
    g, tw = pair(lib, t, roster, net, 2, 64, io, lap_target=0)
    assert g.progress()[:, 4].all()
    noise = np.random.default_rng(2).standard_normal((T, 2, 2, 2)).astype(np.float32)
    out, count = replay("finished", g, tw, roster, net, T, std=(0.5, 0.5), clip=((0.5, 2.0), (-1.0, 1.0)), noise=noise)
    assert count["finished_rows"] == T * 4
    assert (out["mean"] == 0).all() and (out["action"] == 0).all(), "a finished car reads mean = action = (0, 0), whatever the clip"
    assert out["terminated"].all()
    x, m, a = model_rows(net, dict(scans=g.lidar().reshape(2, 2, -1), pose=g.pose().reshape(2, 2, -1), ctrl=g.ctrl().reshape(2, 2, -1),
                                   finished=np.zeros((2, 2), dtype=bool)), (0.0, 0.0), None, (0.5, -1.0), (2.0, 1.0))
    assert np.abs(m).max() > 0, "the network itself would have proposed something"
    g.close(); tw.close()
    # lap_target 1, two agents per env: car 0 of every env is brought to the last point of its lap and finishes during the call, while
    # car 1 races on beside it -- finished and live waves in one workgroup, and an env that does not terminate
    from tests import device_twin
    T1 = 24
    g, tw = pair(lib, t, roster, net, 3, 64, dict(max_episode_steps=0, action_repeat=10, auto_reset=False), lap_target=1)
    device_twin.teleport([g, tw], [t.path] * 3, [0, 1, 2], [0], 2)
    noise = np.random.default_rng(4).standard_normal((T1, 3, 2, 2)).astype(np.float32)
    out, count = replay("one car finishes", g, tw, roster, net, T1, std=(0.3, 0.2), clip=((0.5, 3.0), (-0.5, 0.5)), noise=noise)
    idle = (out["mean"] == 0).all(axis=3) & (out["action"] == 0).all(axis=3)          # [T, n_envs, 2]
    assert not idle[0].any(), "nobody has finished when the call begins"
    assert idle[-1, :, 0].all() and not idle[:, :, 1].any(), f"car 0 finishes during the call, car 1 races on: {idle[:, :, 0].sum(axis=0)}"
    assert g.progress()[0::2, 4].all() and not g.progress()[1::2, 4].any()
    assert 0 < count["finished_rows"] < T1 * 3 and not out["terminated"].any()
    assert np.abs(out["inputs"][-1, :, 0]).max() > 0, "a finished car's inputs are recorded all the same"
    g.close(); tw.close()
    # A diverged network: an infinite weight in the last layer, in front of an identity output.  Where it meets a hidden output of exactly
    # 0 (a relu neuron with a large negative bias) the sum is a NaN: the mean shows it, the guard gives (0, 0).  Where it meets hidden
    # outputs that are not 0 the mean is +-infinity, and by the written order -- the clip, then the guard -- the action is the clip's bound.
    for what, dead in (("diverged to a NaN", True), ("diverged to infinity", False)):
        bad = dict(driver_net(42, hidden_act="relu"), out_act="identity")
        bad["layers"] = [(W.copy(), b.copy()) for W, b in bad["layers"]]
        if dead:
            bad["layers"][0][1][0] = -1.0e6
        else:
            bad["layers"][0][0][0], bad["layers"][0][1][0] = 0.0, 1.0          # that hidden output is exactly 1
        bad["layers"][-1][0][1, 0] = np.inf
        g, tw = pair(lib, t, roster, bad, 3, 64, dict(max_episode_steps=0, action_repeat=1, auto_reset=True))
        noise = np.random.default_rng(2).standard_normal((T, 3, 2, 2)).astype(np.float32)
        out, _ = replay(what, g, tw, roster, bad, T, std=(0.5, 0.5), clip=((0.5, 2.0), (-1.0, 1.0)), noise=noise)
        assert np.isfinite(out["mean"][..., 0]).all() and np.abs(out["mean"][..., 0]).max() > 0, "the other mean is what it is"
        if dead:
            assert np.isnan(out["mean"][..., 1]).all(), "the mean is not guarded"
            assert (out["action"] == 0).all(), "a diverged network acts as the null driver"
        else:
            assert np.isposinf(out["mean"][..., 1]).all(), "the mean is not guarded"
            assert (out["action"][..., 1] == 1.0).all() and (out["action"][..., 0] >= 0.5).all(), "an infinite mean is clipped to the bound"
        assert np.isfinite(g.pose()).all() and np.isfinite(out["action"]).all()
        g.close(); tw.close()
    print("finished and diverged ok")


def reset_dynamics(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = driver_net(51)
    roster, n_envs, T = ["agent", "nidc"], 5, 10
    io = dict(max_episode_steps=4, action_repeat=1, auto_reset=True)
    g, tw = pair(lib, t, roster, net, n_envs, 64, io)
    offset_steps((g, tw), [1, 0, 1, 0, 1])            # envs 1 and 3 end at decisions 1, 5, 9; the others at 3 and 7
    rng = np.random.default_rng(6)
    rows = g.base_dynamics() * rng.uniform(0.8, 1.25, (T, n_envs, 2, 8))
    rows[3, 2, 0, 0] = -1.0                           # an invalid row where env 2 ends: rejected, the old row stays
    rows[2, 1, 1, 2] = np.nan                         # an invalid row where nobody ends: never looked at
    noise = rng.standard_normal((T, n_envs, 1, 2)).astype(np.float32)
    out, count = replay("reset dynamics", g, tw, roster, net, T, std=(0.3, 0.2), clip=((0.0, 4.0), (-0.5, 0.5)), noise=noise, dyn_rows=rows)
    ended = (out["terminated"] | out["truncated"]).astype(bool)
    assert [list(np.flatnonzero(ended[:, e])) for e in range(n_envs)] == [[3, 7], [1, 5, 9], [3, 7], [1, 5, 9], [3, 7]], ended.T
    got, rejected = g.dynamics()
    want_twin, rejected_twin = tw.dynamics()
    np.testing.assert_array_equal(got, want_twin)
    assert rejected == rejected_twin == 1, (rejected, rejected_twin)
    want = np.stack([rows[7, 0], rows[9, 1], rows[7, 2], rows[9, 3], rows[7, 4]]).reshape(n_envs * 2, 8)
    np.testing.assert_array_equal(got, want, err_msg="the rows of the last decision at which the env ended")
    g.close(); tw.close()
    # before any env has ended the table is on, with the handle's own values; ended envs alone take rows
    g, tw = pair(lib, t, roster, net, n_envs, 64, io)
    offset_steps((g, tw), [1, 0, 1, 0, 1])
    out, _ = replay("reset dynamics, two decisions", g, tw, roster, net, 2, dyn_rows=rows[:2].copy())
    got, rejected = g.dynamics()
    base = np.broadcast_to(g.base_dynamics(), (n_envs, 2, 8)).copy()
    base[[1, 3]] = rows[1, [1, 3]]
    np.testing.assert_array_equal(got, base.reshape(-1, 8), err_msg="the others are untouched")
    assert rejected == 0
    # auto_reset off: a state error before anything is enqueued
    g.device_io_config(roster, max_episode_steps=4, action_repeat=1, auto_reset=False)
    before = records(g)
    buf = Buffers(2, n_envs, 1, 17)
    d = torch.from_numpy(rows[:2].copy()).to(DEV)
    try:
        buf.collect(g, 2, reset_dynamics=d.data_ptr())
    except capi.FtgpError as x:
        assert x.code == ERR_STATE and "auto_reset" in str(x), x
    else:
        raise AssertionError("reset_dynamics without auto_reset was accepted")
    np.testing.assert_array_equal(records(g), before)
    g.close(); tw.close()
    print("reset dynamics ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = driver_net(61)
    n_envs, T = 3, 4
    with capi.Env(lib, t, n_envs=n_envs, cars_per_env=2, n_rays=64, spawn_mode=1, seed=5) as g:
        buf = Buffers(T, n_envs, 1, 17, next_inputs=True)
        noise = zeros((T, n_envs, 1, 2))
        dyn = zeros((T, n_envs, 2, 8), torch.float64)
        host = np.zeros(1 << 16, dtype=np.float32)
        # A buffer too small.  The check knows an allocation's extent from the runtime, and torch carves small tensors out of larger
        # allocations: 12 MB is an allocation of its own, and an address near its end has that much room and no more.
        own = zeros(3 << 20)
        end = own.data_ptr() + 4 * (3 << 20)

        def args(**over):
            c = capi.collect_args(T, 0, (0.1, 0.1), ((0.0, 3.0), (-0.5, 0.5)))
            for name in ("inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs"):
                setattr(c, name, getattr(buf, name).data_ptr())
            c.noise = noise.data_ptr()
            for k, v in over.items():
                if isinstance(v, tuple):
                    getattr(c, k)[v[0]] = v[1]
                else:
                    setattr(c, k, v)
            return c

        def refused(code, word, **over):
            before = records(g)
            torch.cuda.synchronize()
            rc = lib.fn("collect_device")(g.h, args(**over))
            assert rc == code, (over, rc, lib.last_error())
            assert word in lib.last_error(), (over, lib.last_error())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(records(g), before, err_msg=f"the handle's state after a refusal ({over})")

        refused(ERR_STATE, "ftgp_device_io_config")                         # before ftgp_device_io_config
        g.device_io_config(["agent", "nidc"], max_episode_steps=3, action_repeat=1, auto_reset=True)
        refused(ERR_STATE, "slot 0")                                        # the slot is not defined
        set_net(g, 0, net)
        refused(ERR_STATE, "slot 2", slot=2)
        refused(ERR_ARG, "slot", slot=4); refused(ERR_ARG, "slot", slot=-1)
        refused(ERR_ARG, "n_decisions", n_decisions=0); refused(ERR_ARG, "n_decisions", n_decisions=-3)
        for bad in (-0.5, float("nan"), float("inf")):
            refused(ERR_ARG, "std[0]", std=(0, bad)); refused(ERR_ARG, "std[1]", std=(1, bad))
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(ERR_ARG, "lo[1]", lo=(1, bad)); refused(ERR_ARG, "hi[0]", hi=(0, bad))
        refused(ERR_ARG, "lo[0]", lo=(0, 3.5)); refused(ERR_ARG, "lo[1]", hi=(1, -0.75))
        refused(ERR_ARG, "reserved", reserved=1)
        for name in ("noise", "inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs", "reset_dynamics"):
            refused(ERR_ARG, name, **{name: host.ctypes.data})              # a host pointer
            refused(ERR_ARG, name, **{name: end - 8})                       # a buffer too small: 8 bytes of room
        for name in ("inputs", "mean", "action", "reward", "terminated", "truncated"):
            refused(ERR_ARG, name, **{name: None})
        refused(ERR_ARG, "reward", reward=end - 4 * n_envs)                 # room for one decision, too small for T
        refused(ERR_ARG, "mean", mean=end - 4 * 2 * n_envs * (T - 1))       # room for T - 1
        refused(ERR_ARG, "n_decisions", n_decisions=-(2 ** 31))
        refused(ERR_ARG, "noise", n_decisions=2 ** 31 - 1)                  # the T-fold size in size_t: far beyond the buffer
        g.device_io_config(["agent", "net3"], max_episode_steps=3, action_repeat=1, auto_reset=True)
        refused(ERR_STATE, "slot 3")                                        # a roster slot whose network is not defined
        g.device_io_config(["agent", "nidc"], max_episode_steps=3, action_repeat=1, auto_reset=False)
        refused(ERR_STATE, "auto_reset", reset_dynamics=dyn.data_ptr())
        # and the call the refusals were variations of is accepted
        g.device_io_config(["agent", "nidc"], max_episode_steps=3, action_repeat=1, auto_reset=True)
        assert lib.fn("collect_device")(g.h, args(reset_dynamics=dyn.data_ptr())) == 0, lib.last_error()
        torch.cuda.synchronize()
        assert g.steps().max() == 1 and buf.truncated.cpu().numpy()[2].all()
    # Four cars' rays share a workgroup's 64 KiB of LDS: a slot whose beams cover 4048 rays is the widest that runs, one more beam is
    # refused before anything is enqueued
    with capi.Env(lib, t, n_envs=2, n_rays=8192, spawn_mode=1, seed=5) as g:
        g.device_io_config(["agent"], max_episode_steps=0, action_repeat=1, auto_reset=True)
        rng = np.random.default_rng(8)
        for slot, n_beams in ((0, 253), (1, 254)):
            set_net(g, slot, nm.random_net(rng, (n_beams, 2), pool=16, max_range=8.0, beam_first=64, out_act="identity"))
        wide = Buffers(2, 2, 1, 254)
        before = records(g)
        try:
            wide.collect(g, 2, slot=1)
        except capi.FtgpError as x:
            assert x.code == ERR_ARG and "LDS" in str(x) and "4064" in str(x), x
        else:
            raise AssertionError("a slot whose rays do not fit LDS was accepted")
        np.testing.assert_array_equal(records(g), before)
    t_small = load_track("small-circle")
    kw = dict(n_envs=2, n_rays=8192, spawn_mode=1, seed=5)
    g, tw = (capi.Env(lib, t_small, **kw) for _ in range(2))
    for e in (g, tw):
        e.device_io_config(["agent"], max_episode_steps=0, action_repeat=1, auto_reset=True)
    widest = nm.random_net(np.random.default_rng(8), (253, 2), pool=16, max_range=8.0, beam_first=64, out_act="identity")
    set_net(g, 0, widest)
    replay("the widest slot", g, tw, ["agent"], widest, 3, std=(0.1, 0.1), clip=((0.0, 2.0), (-0.5, 0.5)),
           noise=np.random.default_rng(9).standard_normal((3, 2, 1, 2)).astype(np.float32))
    g.close(); tw.close()
    print("errors ok")


def vec_env(opt):
    from ft_grandprix_amd.net import NetSpec
    from ft_grandprix_amd.vec import DeviceVecEnv, Rollout
    net = driver_net(71)
    spec = NetSpec(net["layers"], **fields(net))
    kw = dict(n_envs=6, n_rays=64, cars_per_env=2, roster=["agent", "nidc"], action_repeat=2, max_episode_steps=8, scan_pool=4,
              scan_max_range=3.0, state=True, spawn_mode=1, seed=9)
    a = DeviceVecEnv("small-circle", nets={0: spec}, **kw)
    b = DeviceVecEnv("small-circle", **kw)
    a.reset(); b.reset()
    T, std, clip = 6, (0.4, 0.2), ((0.0, 3.0), (-0.4, 0.4))
    side = torch.cuda.Stream()
    roll, kept = None, None
    for round_ in range(3):
        # on a stream of its own, the noise produced on it right before the call: the library must wait for it
        with torch.cuda.stream(side):
            gen = torch.Generator(device=a.device); gen.manual_seed(100 + round_)
            big = torch.randn((2048, 2048), generator=gen, device=a.device)
            for _ in range(20):
                big = torch.tanh(big @ big)                                 # work in front of the noise on that stream
            noise = (torch.randn((T, 6, 1, 2), generator=gen, device=a.device) + 0.0 * big[0, 0]).contiguous()
            roll = a.collect(T, std=std, clip=clip, noise=noise, next_inputs=True, out=roll)
            got = {k: getattr(roll, k).cpu().numpy() for k in ("inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs")}
            nz = noise.cpu().numpy()
        assert isinstance(roll, Rollout) and roll.noise is noise
        if kept is None:
            kept = {k: getattr(roll, k).data_ptr() for k in got}
        assert kept == {k: getattr(roll, k).data_ptr() for k in got}, "out= reuses the tensors"
        assert got["inputs"].shape == (T, 6, 1, 17) and got["mean"].shape == got["action"].shape == (T, 6, 1, 2)
        assert got["reward"].shape == (T, 6, 1) and got["terminated"].shape == got["truncated"].shape == (T, 6)
        assert roll.terminated.dtype == torch.bool and got["next_inputs"].shape == got["inputs"].shape
        want = cmod.action(got["mean"].reshape(-1, 2), std, nz.reshape(-1, 2), (0.0, -0.4), (3.0, 0.4)).reshape(T, 6, 1, 2)
        cmod.assert_same_bits(got["action"], want, f"round {round_}: the action holds the noise drawn on the caller's stream")
        assert np.abs(nz).max() > 0 and not cmod.same_bits(got["action"], got["mean"])
        # the twin env: the same actions one step at a time, then a step of the caller's on both
        for t in range(T):
            x_b = np.concatenate([b.obs[:, :, 2:14].cpu().numpy(), b.state[:, :, :5].cpu().numpy()], axis=2)
            cmod.assert_same_bits(got["inputs"][t], x_b, f"round {round_}: inputs[{t}] are what an agent is given")
            _, r, te, tr, _ = b.step(roll.action[t].to(torch.device(a.device)).contiguous())
            cmod.assert_same_bits(got["reward"][t], r.cpu().numpy(), f"round {round_}: reward[{t}]")
            assert torch.equal(te.cpu(), roll.terminated[t].cpu()) and torch.equal(tr.cpu(), roll.truncated[t].cpu())
        assert torch.equal(a.obs.cpu(), b.obs.cpu()) and torch.equal(a.state.cpu(), b.state.cpu()), "obs and state after collect"
        act = torch.tensor([1.5, 0.1 * round_], device=a.device).expand(6, 1, 2).contiguous()
        for _ in range(3):
            oa, ra, ta, tra, ia = a.step(act)
            ob, rb, tb, trb, ib = b.step(act)
            assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(tra, trb) and torch.equal(ia["state"], ib["state"])
    ended = int((roll.terminated | roll.truncated).sum())
    np.testing.assert_array_equal(a.env.pose(), b.env.pose())
    # noise=True draws on the device; noise=None explores nothing; a slot that is not defined, a wrong out
    r2 = a.collect(3, noise=True)
    assert r2.noise.shape == (3, 6, 1, 2) and r2.next_inputs is None and float(r2.noise.abs().max()) > 0
    drawn, first = r2.noise.data_ptr(), r2.noise.clone()
    r2 = a.collect(3, noise=True, out=r2)
    assert r2.noise.data_ptr() == drawn and not torch.equal(r2.noise, first), "noise=True with out= draws into the tensor it has"
    want = cmod.action(r2.mean.cpu().numpy().reshape(-1, 2), (0.0, 0.0), r2.noise.cpu().numpy().reshape(-1, 2), (-1e30, -1e30), (1e30, 1e30))
    cmod.assert_same_bits(r2.action.cpu().numpy().reshape(-1, 2), want, "std = 0: the action is the mean, whatever the noise")
    r3 = a.collect(3)
    assert r3.noise is None and torch.equal(r3.action, r3.mean)
    for bad in (lambda: a.collect(3, slot=1), lambda: a.collect(4, out=r3), lambda: a.collect(3, noise=torch.zeros(3)),
                lambda: a.collect(0), lambda: a.collect(3, std=(-1.0, 0.0)), lambda: a.collect(3, clip=((1.0, 0.0), (0.0, 1.0)))):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad collect() was accepted")
    a.close(); b.close()
    # with randomize_dynamics: the rows drawn up front, the mirror follows the device table
    c = DeviceVecEnv("small-circle", nets={0: spec}, randomize_dynamics=dict(mass=(4.0, 7.0), friction=(0.6, 1.2)), dynamics_seed=3,
                     **{**kw, "max_episode_steps": 4, "action_repeat": 1})
    c.reset()
    c.collect(10, noise=True)
    kept_rows = c._collect_rows.data_ptr()
    c.collect(10, noise=True)
    assert c._collect_rows.data_ptr() == kept_rows, "the dynamics rows of a collect are drawn into one block"
    torch.cuda.synchronize()
    rows, rejected = c.env.dynamics()
    np.testing.assert_array_equal(c.dynamics.cpu().numpy().reshape(-1, 8), rows, err_msg="the dynamics mirror after collect")
    assert rejected == 0
    c.close()
    print(f"vec env ok ({ended} ends in the last round)")


SCENARIOS = {"replay_and_model": replay_and_model, "next_inputs": next_inputs, "against_roster": against_roster, "rules": rules,
             "finished_and_diverged": finished_and_diverged, "reset_dynamics": reset_dynamics, "errors": errors, "vec_env": vec_env}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
