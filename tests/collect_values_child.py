"""Child process of tests/test_collect_values.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/collect_values_child.py <scenario> [json options]

The criterion throughout (include/ftgp.h "Collected rollouts with values"): every buffer of c and the handle after
ftgp_collect_values_device are, to the bit, what plain ftgp_collect_device leaves on a twin handle; value and next_value are the numpy
model of the header's text (tests/collect_values_model.py) on the recorded inputs and next_inputs; advantage and ret are the model's
scan.  No tolerance anywhere.
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
from tests import collect_child as cc  # noqa: E402
from tests import collect_model as cmod  # noqa: E402
from tests import collect_values_model as vm  # noqa: E402
from tests import net_model as nm  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
DEV = "cuda"
F = np.float32
zeros = cc.zeros
C_BUFFERS = ("inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs")


def set_value_net(env, slot, vnet):
    env.set_value_net(slot, vnet["layers"], **vm.value_fields(vnet))


class VBuffers(cc.Buffers):
    """The buffers of one ftgp_collect_values_device call."""

    def __init__(self, T, n_envs, n_ext, n_in, next_inputs=True, advantage=True):
        super().__init__(T, n_envs, n_ext, n_in, next_inputs=next_inputs)
        lead = (T, n_envs, n_ext)
        self.value, self.next_value = zeros(lead), zeros(lead)
        self.advantage, self.ret = (zeros(lead), zeros(lead)) if advantage else (None, None)

    def collect_values(self, env, T, gamma=0.99, lam=0.95, **kw):
        env.collect_values_device(T, self.inputs.data_ptr(), self.mean.data_ptr(), self.action.data_ptr(), self.reward.data_ptr(),
                                  self.terminated.data_ptr(), self.truncated.data_ptr(), self.value.data_ptr(), self.next_value.data_ptr(),
                                  advantage=0 if self.advantage is None else self.advantage.data_ptr(),
                                  ret=0 if self.ret is None else self.ret.data_ptr(), gamma=gamma, lam=lam,
                                  next_inputs=0 if self.next_inputs is None else self.next_inputs.data_ptr(), **kw)


def pair(lib, track, roster, net, n_envs, n_rays, io, setup=None, **kw):
    """Two handles configured alike, the network in slot 0 of both: the twin runs plain ftgp_collect_device."""
    envs = []
    for _ in range(2):
        e = capi.Env(lib, track, n_envs=n_envs, cars_per_env=len(roster), n_rays=n_rays, spawn_mode=1, seed=5, **kw)
        e.device_io_config(roster, **io)
        if setup:
            setup(e)
        cc.set_net(e, 0, net)
        envs.append(e)
    return envs


def same_handles(what, g, tw):
    np.testing.assert_array_equal(cc.records(g), cc.records(tw), err_msg=f"{what}: the env-state records at the end")
    np.testing.assert_array_equal(g.episodes(), tw.episodes(), err_msg=f"{what}: episodes")
    for name, a, b in (("lidar", g.lidar(), tw.lidar()), ("pose", g.pose(), tw.pose()), ("ctrl", g.ctrl(), tw.ctrl()),
                       ("progress", g.progress(), tw.progress()), ("steps", g.steps(), tw.steps())):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name} at the end")


def compare(what, g, tw, vnet, T, n_ext, *, gamma=0.99, lam=0.95, seed=7, **kw):
    """T decisions with values on g, plain on the twin; everything compared.  Returns g's host copies."""
    n, n_in = g.n_envs, g._net_n_in(0)
    noise = torch.from_numpy(np.random.default_rng(seed).standard_normal((T, n, n_ext, 2)).astype(F)).to(DEV)
    bg, bt = VBuffers(T, n, n_ext, n_in), cc.Buffers(T, n, n_ext, n_in, next_inputs=True)
    bg.collect_values(g, T, gamma, lam, noise=noise.data_ptr(), **kw)
    bt.collect(tw, T, noise=noise.data_ptr(), **kw)
    torch.cuda.synchronize()
    og, ot = bg.host(), bt.host()
    for name in C_BUFFERS:
        cmod.assert_same_bits(og[name].astype(F), ot[name].astype(F), f"{what}: {name} against plain ftgp_collect_device")
    same_handles(what, g, tw)
    cmod.assert_same_bits(og["value"], vm.value(vnet, og["inputs"]), f"{what}: value against the model on inputs")
    cmod.assert_same_bits(og["next_value"], vm.value(vnet, og["next_inputs"]), f"{what}: next_value against the model on next_inputs")
    adv, ret = vm.gae(og["reward"], og["value"], og["next_value"], og["terminated"], og["truncated"], gamma, lam)
    cmod.assert_same_bits(og["advantage"], adv, f"{what}: advantage against the model's scan")
    cmod.assert_same_bits(og["ret"], ret, f"{what}: ret against the model's scan")
    return og


def bootstrap_rows(what, out):
    """next_value[t] == value[t + 1] to the bit wherever the env did not end at t; returns how many rows of ended envs differ."""
    ended = (out["terminated"] | out["truncated"]).astype(bool)
    differ = 0
    for t in range(len(ended) - 1):
        keep = ~ended[t]
        cmod.assert_same_bits(out["next_value"][t][keep], out["value"][t + 1][keep], f"{what}: next_value[{t}] == value[{t + 1}] without an end")
        a, b = out["next_value"][t][ended[t]], out["value"][t + 1][ended[t]]
        differ += int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())
    return differ


def replay_and_model(opt):
    lib = capi.load()
    t = load_track("small-circle")
    T = 12
    io = dict(max_episode_steps=5, action_repeat=1, auto_reset=True)
    cases = nm.eval_cases()
    rng = np.random.default_rng(23)
    shapes = {"one_layer 7x1": (["agent"], 7, 64, cases["one_layer"][1][0], (0.4, 0.3), ((0.2, 1.0), (-1.5, -0.5)),
                                [vm.random_value_net(rng, (12, 1), out_scale=2.0, out_offset=0.5)]),
              "wide 3x3": (["agent", "fast", "agent"], 3, 1080, cases["mlp_tanh"][1][0], (1.0, 0.3), ((0.5, 4.5), (-0.3, 0.3)),
                           [vm.random_value_net(rng, (85, 128, 1), out_scale=3.0), vm.random_value_net(rng, (85, 65, 1), hidden_act="relu", out_act="tanh"),
                            vm.random_value_net(rng, (85, 1, 1), out_offset=-1.0), vm.random_value_net(rng, (85, 128, 65, 1, 1), gain=2.0)])}
    roster, n_envs, n_rays, net, std, clip, vnets = shapes[opt["only"]]
    n_ext = roster.count("agent")
    assert (n_envs * n_ext) % 4 != 0
    g, tw = pair(lib, t, roster, net, n_envs, n_rays, io)
    for i, vnet in enumerate(vnets):
        what = f"{opt['only']}, value net {[W.shape[0] for W, _ in vnet['layers']]}"
        set_value_net(g, 0, vnet)
        out = compare(what, g, tw, vnet, T, n_ext, std=std, clip=clip, seed=7 + i)
        ended = (out["terminated"] | out["truncated"]).astype(bool)
        assert ended.sum() >= 2 * n_envs and ended[:-1].any() and not ended.all(), f"{what}: envs end inside the rollout: {ended.sum()}"
        lo, hi = F([clip[0][0], clip[1][0]]), F([clip[0][1], clip[1][1]])
        at_bound = (out["action"] == lo) | (out["action"] == hi)
        assert at_bound.any() and not at_bound.all(), f"{what}: the clip binds for some rows only"
        assert np.isfinite(out["value"]).all() and np.unique(out["value"]).size > T, f"{what}: the values vary"
        assert bootstrap_rows(what, out) > 0, f"{what}: no row of an ended env tells next_value from the value after the reset"
        print(f"{what}: {int(ended.sum())} ends")
    g.close(); tw.close()
    print("replay and model ok")


def bootstrap(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = nm.eval_cases()["mlp_tanh"][1][1]
    vnet = vm.random_value_net(np.random.default_rng(29), (85, 37, 1))
    roster, n_envs, T = ["agent", "agent"], 3, 9
    io = dict(max_episode_steps=4, action_repeat=1, auto_reset=True)
    g, h = pair(lib, t, roster, net, n_envs, 1080, io)
    for e in (g, h):
        set_value_net(e, 0, vnet)
    cc.offset_steps((g, h), [1, 0, 1])
    noise = torch.from_numpy(np.random.default_rng(9).standard_normal((T, n_envs, 2, 2)).astype(F)).to(DEV)
    kw = dict(std=(0.5, 0.2), clip=((0.0, 5.0), (-0.5, 0.5)), noise=noise.data_ptr())
    with_x, without = VBuffers(T, n_envs, 2, 85), VBuffers(T, n_envs, 2, 85, next_inputs=False)
    with_x.collect_values(g, T, **kw)
    without.collect_values(h, T, **kw)
    torch.cuda.synchronize()
    a, b = with_x.host(), without.host()
    assert "next_inputs" not in b
    for name in ("inputs", "mean", "action", "reward", "terminated", "truncated", "value", "next_value", "advantage", "ret"):
        cmod.assert_same_bits(a[name].astype(F), b[name].astype(F), f"{name} without next_inputs")
    cmod.assert_same_bits(b["next_value"], vm.value(vnet, a["next_inputs"]), "next_value against the model on the other handle's next_inputs")
    assert (a["terminated"] | a["truncated"]).sum() >= 4 and bootstrap_rows("bootstrap", b) > 0
    same_handles("bootstrap", g, h)
    g.close(); h.close()
    print("bootstrap ok")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_gae(env, case, reward=None):
    T, n, k = case["reward"].shape
    r, v, nv = dev(case["reward"] if reward is None else reward), dev(case["value"]), dev(case["next_value"])
    te, tr = dev(case["terminated"]), dev(case["truncated"])
    adv, ret = zeros((T, n, k)), zeros((T, n, k))
    env.gae_device(T, r.data_ptr(), v.data_ptr(), nv.data_ptr(), te.data_ptr(), tr.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                   gamma=case["gamma"], lam=case["lam"])
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy()


def gae(opt):
    lib = capi.load()
    t = load_track("small-circle")
    cases = vm.scan_cases()
    hand, A64, R64 = vm.hand_row()
    with capi.Env(lib, t, n_envs=7, n_rays=64, spawn_mode=1, seed=5) as g7, \
            capi.Env(lib, t, n_envs=65, cars_per_env=2, n_rays=64, spawn_mode=1, seed=5) as g130, \
            capi.Env(lib, t, n_envs=1, n_rays=64, spawn_mode=1, seed=5) as g1:
        g7.device_io_config(["agent"], max_episode_steps=20, action_repeat=4, auto_reset=True)
        g7.device_io_frame(True, n_ahead=0, stride=1, dense_progress=True)          # a dense reward: no row of zeros to scale
        g130.device_io_config(["agent", "agent"], max_episode_steps=5, action_repeat=1, auto_reset=True)
        g1.device_io_config(["agent"], max_episode_steps=5, action_repeat=1, auto_reset=True)
        for name, c in sorted(cases.items()):
            env = g130 if c["reward"].shape[1:] == (65, 2) else g7
            assert c["reward"].shape[1:] in ((65, 2), (7, 1))
            adv, ret = run_gae(env, c)
            want_adv, want_ret = vm.gae(c["reward"], c["value"], c["next_value"], c["terminated"], c["truncated"], c["gamma"], c["lam"])
            cmod.assert_same_bits(adv, want_adv, f"{name}: advantage")
            cmod.assert_same_bits(ret, want_ret, f"{name}: ret")
        adv, ret = run_gae(g1, hand)
        cmod.assert_same_bits(adv, A64.astype(F), "the row written out by hand")
        cmod.assert_same_bits(ret, R64.astype(F), "the row written out by hand: ret")
        # a collected rollout: the entry alone gives the call's own advantage, and the model's on rewards scaled by one half
        net = cc.driver_net(21)
        vnet = vm.random_value_net(np.random.default_rng(31), (17, 16, 1))
        cc.set_net(g7, 0, net); set_value_net(g7, 0, vnet)
        T = 12
        buf = VBuffers(T, 7, 1, 17)
        buf.collect_values(g7, T, 0.97, 0.9, std=(0.3, 0.2), clip=((0.0, 4.0), (-0.5, 0.5)))
        torch.cuda.synchronize()
        out = buf.host()
        case = dict(reward=out["reward"], value=out["value"], next_value=out["next_value"], terminated=out["terminated"], truncated=out["truncated"],
                    gamma=0.97, lam=0.9)
        assert out["truncated"].any() and np.abs(out["reward"]).max() > 0
        adv, ret = run_gae(g7, case)
        cmod.assert_same_bits(adv, out["advantage"], "ftgp_gae_device on a collected rollout: its advantage")
        cmod.assert_same_bits(ret, out["ret"], "ftgp_gae_device on a collected rollout: its ret")
        half = (out["reward"] * F(0.5)).astype(F)
        adv, ret = run_gae(g7, case, reward=half)
        want_adv, want_ret = vm.gae(half, out["value"], out["next_value"], out["terminated"], out["truncated"], 0.97, 0.9)
        cmod.assert_same_bits(adv, want_adv, "rewards scaled by one half: advantage")
        cmod.assert_same_bits(ret, want_ret, "rewards scaled by one half: ret")
        assert not cmod.same_bits(adv, out["advantage"])
    print("gae ok")


def finished_and_diverged(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = cc.driver_net(41)
    roster, T = ["agent", "agent"], 4
    io = dict(max_episode_steps=0, action_repeat=1, auto_reset=False)
    vnet = vm.random_value_net(np.random.default_rng(37), (17, 16, 1), out_offset=0.25)
    # lap_target 0: every car has finished from the start -- the policy is not looked at, the value is
    g, tw = pair(lib, t, roster, net, 2, 64, io, lap_target=0)
    assert g.progress()[:, 4].all()
    set_value_net(g, 0, vnet)
    out = compare("finished", g, tw, vnet, T, 2, std=(0.5, 0.5), clip=((0.5, 2.0), (-1.0, 1.0)))
    assert (out["mean"] == 0).all() and (out["action"] == 0).all(), "a finished car reads mean = action = (0, 0)"
    assert np.isfinite(out["value"]).all() and (out["value"] != 0).all() and (out["next_value"] != 0).all(), "its value is evaluated all the same"
    g.close(); tw.close()
    # A diverged critic: an infinite weight in the last layer.  Where it meets a hidden output of exactly 0 (a relu neuron with a large
    # negative bias) the value is a NaN; where it meets a hidden output of exactly 1 it is infinite.  No guard: the record shows it, and
    # the action and the handle are what they are without a critic.
    for what, dead in (("diverged to a NaN", True), ("diverged to infinity", False)):
        bad = vm.random_value_net(np.random.default_rng(38), (17, 16, 1), hidden_act="relu")
        if dead:
            bad["layers"][0][1][0] = -1.0e6
        else:
            bad["layers"][0][0][0], bad["layers"][0][1][0] = 0.0, 1.0
        bad["layers"][-1][0][0, 0] = np.inf
        g, tw = pair(lib, t, roster, net, 3, 64, dict(max_episode_steps=3, action_repeat=1, auto_reset=True))
        set_value_net(g, 0, bad)
        out = compare(what, g, tw, bad, T, 2, std=(0.5, 0.5), clip=((0.5, 2.0), (-1.0, 1.0)))
        for name in ("value", "next_value", "advantage", "ret"):
            assert (np.isnan(out[name]).all() if dead else not np.isfinite(out[name]).any()), f"{what}: {name} = {out[name].ravel()[:4]}"
        if not dead:
            assert np.isposinf(out["value"]).all()
        assert np.isfinite(out["action"]).all() and np.abs(out["action"]).max() > 0 and np.isfinite(g.pose()).all()
        g.close(); tw.close()
    print("finished and diverged ok")


def expect(code, word, fn):
    try:
        fn()
    except capi.FtgpError as x:
        assert x.code == code and word in str(x), x
    else:
        raise AssertionError(f"accepted where error {code} ({word}) was expected")


def refresh(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net, net2 = cc.driver_net(51), cc.driver_net(52)
    rng = np.random.default_rng(41)
    v1, v2 = vm.random_value_net(rng, (17, 65, 1)), vm.random_value_net(rng, (17, 65, 1))
    roster, T = ["agent"], 6
    g, tw = pair(lib, t, roster, net, 5, 64, dict(max_episode_steps=4, action_repeat=1, auto_reset=True))
    set_value_net(g, 0, v1)
    kw = dict(std=(0.3, 0.2), clip=((0.0, 4.0), (-0.5, 0.5)))
    compare("before the refresh", g, tw, v1, T, 1, **kw)
    # new parameters produced on a side stream behind a pile of work, handed over on that stream, and a collect on the default stream
    # right behind it: nothing synchronises in between
    from ft_grandprix_amd.net import ValueSpec
    flat2 = ValueSpec(v2["layers"], **vm.value_fields(v2)).flat_params()
    side = torch.cuda.Stream()
    n, n_in = 5, 17
    noise = dev(np.random.default_rng(3).standard_normal((T, n, 1, 2)).astype(F))
    bg, bt = VBuffers(T, n, 1, n_in), cc.Buffers(T, n, 1, n_in, next_inputs=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn((2048, 2048), device=DEV)
        for _ in range(20):
            big = torch.tanh(big @ big)
        params = (torch.from_numpy(flat2).to(DEV) + 0.0 * big[0, 0]).contiguous()
        g.set_value_net_device(0, params.data_ptr(), side.cuda_stream)
    bg.collect_values(g, T, noise=noise.data_ptr(), **kw)
    bt.collect(tw, T, noise=noise.data_ptr(), **kw)
    torch.cuda.synchronize()
    og, ot = bg.host(), bt.host()
    for name in C_BUFFERS:
        cmod.assert_same_bits(og[name].astype(F), ot[name].astype(F), f"after the refresh: {name}")
    cmod.assert_same_bits(og["value"], vm.value(v2, og["inputs"]), "after the refresh: the values are the new net's")
    cmod.assert_same_bits(og["next_value"], vm.value(v2, og["next_inputs"]), "after the refresh: next_value")
    assert not cmod.same_bits(og["value"], vm.value(v1, og["inputs"]))
    d, layers = g.get_value_net(0)
    for (W, b), (W2, b2) in zip(layers, v2["layers"]):
        np.testing.assert_array_equal(W, W2); np.testing.assert_array_equal(b, b2)
    assert (d.n_layers, list(d.width)) == (2, [65, 1, 0, 0])
    # ftgp_set_net_device keeps the value net
    from ft_grandprix_amd.net import NetSpec
    p2 = dev(NetSpec(net2["layers"], **cc.fields(net2)).flat_params())
    for e in (g, tw):
        e.set_net_device(0, p2.data_ptr())
    out = compare("after ftgp_set_net_device", g, tw, v2, T, 1, **kw)
    x = out["inputs"].reshape(-1, 17)
    y = nm.forward(x, net2["layers"], net2["hidden_act"], net2["out_act"])
    fin = np.zeros(len(x), dtype=bool)
    cmod.assert_same_bits(out["mean"].reshape(-1, 2), cmod.mean(y, net2["out_scale"], net2["out_offset"]), "the means are the new policy's")
    assert not fin.any()
    # a population leaves it alone as well; ftgp_set_net on the slot clears it
    g.set_net_population(0, np.stack([NetSpec(n_["layers"], **cc.fields(n_)).flat_params() for n_ in (net, net2)]))
    g.get_value_net(0)
    g.set_net_population(0, None)
    g.get_value_net(0)
    before = cc.records(g)
    cc.set_net(g, 0, net)
    expect(ERR_STATE, "value net", lambda: g.get_value_net(0))
    buf = VBuffers(T, n, 1, n_in)
    expect(ERR_STATE, "value net", lambda: buf.collect_values(g, T, **kw))
    expect(ERR_STATE, "value net", lambda: g.set_value_net_device(0, params.data_ptr()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(cc.records(g), before)
    set_value_net(g, 0, v1)
    g.set_value_net(0, None)                                        # desc = NULL clears
    expect(ERR_STATE, "value net", lambda: g.get_value_net(0))
    g.set_value_net(0, None)                                        # ... and clearing nothing is no error
    g.close(); tw.close()
    print("refresh ok")


def population(opt):
    from ft_grandprix_amd.net import NetSpec
    lib = capi.load()
    t = load_track("small-circle")
    members = [cc.driver_net(60 + m) for m in range(4)]
    vnet = vm.random_value_net(np.random.default_rng(43), (17, 32, 1))
    roster, n_envs, T = ["agent"], 8, 6
    g, tw = pair(lib, t, roster, members[0], n_envs, 64, dict(max_episode_steps=4, action_repeat=1, auto_reset=True))
    stack = np.stack([NetSpec(m["layers"], **cc.fields(m)).flat_params() for m in members])
    member = np.array([3, 0, 1, 2, 2, 1, 0, 3], dtype=np.int32)
    for e in (g, tw):
        e.set_net_population(0, stack, member)
    set_value_net(g, 0, vnet)
    out = compare("population", g, tw, vnet, T, 1, std=(0.3, 0.2), clip=((0.0, 4.0), (-0.5, 0.5)))
    for e in range(n_envs):
        m = members[member[e]]
        y = nm.forward(out["inputs"][:, e, 0], m["layers"], m["hidden_act"], m["out_act"])
        cmod.assert_same_bits(out["mean"][:, e, 0], cmod.mean(y, m["out_scale"], m["out_offset"]), f"env {e}: the mean is member {member[e]}'s")
    assert not cmod.same_bits(out["mean"][:, 0], out["mean"][:, 1])
    assert g.get_net_population(0)[0] == 4
    g.close(); tw.close()
    print("population ok")


def rules(opt):
    lib = capi.load()
    small, circle = load_track("small-circle"), load_track("circle")
    scen = opt["only"]
    T = 12
    kw = dict(std=(0.3, 0.2), clip=((0.0, 6.0), (-0.5, 0.5)))
    rng = np.random.default_rng(47)
    if scen == "action repeat 3":
        roster, net = ["agent", "fast", "agent"], cc.driver_net(34)
        g, tw = pair(lib, small, roster, net, 3, 64, dict(max_episode_steps=9, action_repeat=3, auto_reset=True))
        vnet = vm.random_value_net(rng, (17, 16, 1))
    elif scen == "two tracks":
        roster, net = ["agent"], cc.driver_net(34)
        g, tw = pair(lib, [small, circle], roster, net, 5, 64, dict(max_episode_steps=5, action_repeat=2, auto_reset=True), envs_per_track=(2, 3))
        vnet = vm.random_value_net(rng, (17, 16, 1))
    else:
        # frame and rival inputs: 12 beams, 5 state entries, 4 + 2 * 2 frame entries, 4 + 8 * 2 rival entries = 45 inputs
        roster = ["agent", "agent", "nidc"]
        net = dict(nm.random_net(rng, (45, 16, 2), **{**cc.DRIVER, "use_state": False}), n_beams=12, use_state=True, frame=True, lookahead=2,
                   lookahead_stride=3, rivals=True, n_rivals=2)
        g, tw = pair(lib, small, roster, net, 3, 64, dict(max_episode_steps=6, action_repeat=4, auto_reset=True))
        assert g._net_n_in(0) == 45
        vnet = vm.random_value_net(rng, (45, 24, 1))
        w = vnet["layers"][0][0]
        w[:, :17] = 0.0                                              # a critic that looks at the frame and rival entries alone
    n_ext = roster.count("agent")
    set_value_net(g, 0, vnet)
    out = compare(scen, g, tw, vnet, T, n_ext, **kw)
    ended = (out["terminated"] | out["truncated"]).astype(bool)
    assert ended.any() and np.unique(out["value"]).size > T, f"{scen}: {ended.sum()} ends"
    bootstrap_rows(scen, out)
    g.close(); tw.close()
    print(f"rules {scen} ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    net = cc.driver_net(61)
    vnet = vm.random_value_net(np.random.default_rng(53), (17, 16, 1), out_scale=1.5)
    n_envs, T = 3, 4
    with capi.Env(lib, t, n_envs=n_envs, cars_per_env=2, n_rays=64, spawn_mode=1, seed=5) as g:
        buf = VBuffers(T, n_envs, 1, 17)
        host = np.zeros(1 << 16, dtype=F)
        own = zeros(3 << 20)                                            # an allocation of its own: an address near its end has that much room
        end = own.data_ptr() + 4 * (3 << 20)
        d0, flat = capi.value_desc(vnet["layers"], **vm.value_fields(vnet))
        have = [None]                                                   # the value net the handle must hold after a refusal

        def unchanged(before, what):
            torch.cuda.synchronize()
            np.testing.assert_array_equal(cc.records(g), before, err_msg=f"the handle's state after a refusal ({what})")
            if have[0] is None:
                assert lib.fn("get_value_net")(g.h, 0, None, None) == ERR_STATE, what
            else:
                d, layers = g.get_value_net(0)
                assert bytes(d) == bytes(have[0][0]), what
                for (W, b), (W2, b2) in zip(layers, have[0][1]):
                    np.testing.assert_array_equal(W, W2); np.testing.assert_array_equal(b, b2)

        def refused(entry, code, word, *args):
            before = cc.records(g)
            torch.cuda.synchronize()
            rc = lib.fn(entry)(g.h, *args)
            assert rc == code, (entry, word, rc, lib.last_error())
            assert word in lib.last_error(), (entry, word, lib.last_error())
            assert "ftgp_" + entry in lib.last_error() or "ftgp_collect_device" in lib.last_error(), (entry, lib.last_error())     # (c's own errors are ftgp_collect_device's)
            unchanged(before, f"{entry}: {word}")

        def desc(**over):
            d = capi.FtgpValueDesc.from_buffer_copy(bytes(d0))
            for k, v in over.items():
                if isinstance(v, tuple):
                    getattr(d, k)[v[0]] = v[1]
                else:
                    setattr(d, k, v)
            return d

        P = flat.ctypes.data
        # ---- section 3 before ftgp_device_io_config, section 1 on a slot that is not defined
        gae_ok = [None, T, 0.9, 0.9, buf.reward.data_ptr(), buf.value.data_ptr(), buf.next_value.data_ptr(), buf.terminated.data_ptr(),
                  buf.truncated.data_ptr(), buf.advantage.data_ptr(), buf.ret.data_ptr()]
        refused("gae_device", ERR_STATE, "ftgp_device_io_config", *gae_ok)
        g.device_io_config(["agent", "nidc"], max_episode_steps=3, action_repeat=1, auto_reset=True)
        refused("set_value_net", ERR_STATE, "slot 0", 0, desc(), P)
        cc.set_net(g, 0, net)
        # ---- ftgp_set_value_net, first with no value net in force, then with one
        for round_ in range(2):
            refused("set_value_net", ERR_ARG, "slot", 4, desc(), P); refused("set_value_net", ERR_ARG, "slot", -1, desc(), P)
            refused("set_value_net", ERR_STATE, "slot 2", 2, desc(), P)
            refused("set_value_net", ERR_ARG, "n_layers", 0, desc(n_layers=0), P); refused("set_value_net", ERR_ARG, "n_layers", 0, desc(n_layers=5), P)
            refused("set_value_net", ERR_ARG, "width[0]", 0, desc(width=(0, 0)), P); refused("set_value_net", ERR_ARG, "width[0]", 0, desc(width=(0, 129)), P)
            refused("set_value_net", ERR_ARG, "width[1]", 0, desc(width=(1, 2)), P); refused("set_value_net", ERR_ARG, "width[1]", 0, desc(width=(1, 0)), P)
            refused("set_value_net", ERR_ARG, "width[2]", 0, desc(width=(2, 1)), P)
            refused("set_value_net", ERR_ARG, "hidden_act", 0, desc(hidden_act=3), P); refused("set_value_net", ERR_ARG, "out_act", 0, desc(out_act=-1), P)
            refused("set_value_net", ERR_ARG, "out_scale", 0, desc(out_scale=float("inf")), P)
            refused("set_value_net", ERR_ARG, "out_offset", 0, desc(out_offset=float("nan")), P)
            refused("set_value_net", ERR_ARG, "reserved", 0, desc(reserved=1), P)
            refused("set_value_net", ERR_ARG, "params", 0, desc(), None)
            if round_ == 0:
                refused("set_value_net_device", ERR_STATE, "value net", None, 0, own.data_ptr())
                refused("get_value_net", ERR_STATE, "value net", 0, None, None)
                cargs = capi.collect_args(T, 0, (0.1, 0.1), ((0.0, 3.0), (-0.5, 0.5)))
                for name in C_BUFFERS:
                    setattr(cargs, name, getattr(buf, name).data_ptr())
                refused("collect_values_device", ERR_STATE, "value net", cargs,
                        capi.collect_values_args(0.9, 0.9, buf.value.data_ptr(), buf.next_value.data_ptr()))
                set_value_net(g, 0, vnet)
                have[0] = g.get_value_net(0)
        # ---- ftgp_set_value_net_device and ftgp_get_value_net
        refused("set_value_net_device", ERR_ARG, "slot", None, 4, own.data_ptr())
        refused("set_value_net_device", ERR_STATE, "slot 1", None, 1, own.data_ptr())
        refused("set_value_net_device", ERR_ARG, "params", None, 0, None)
        refused("set_value_net_device", ERR_ARG, "params", None, 0, host.ctypes.data)
        refused("set_value_net_device", ERR_ARG, "params", None, 0, end - 8)
        refused("get_value_net", ERR_ARG, "slot", -1, None, None); refused("get_value_net", ERR_ARG, "slot", 4, None, None)
        refused("get_value_net", ERR_STATE, "slot 3", 3, None, None)

        # ---- ftgp_collect_values_device
        def cv(c_over=None, **over):
            c = capi.collect_args(T, 0, (0.1, 0.1), ((0.0, 3.0), (-0.5, 0.5)))
            for name in C_BUFFERS:
                setattr(c, name, getattr(buf, name).data_ptr())
            for k, v in (c_over or {}).items():
                setattr(c, k, v)
            v = capi.FtgpCollectValues(gamma=0.9, lam=0.9)
            for name in ("value", "next_value", "advantage", "ret"):
                setattr(v, name, getattr(buf, name).data_ptr())
            for k, x in over.items():
                if isinstance(x, tuple):
                    getattr(v, k)[x[0]] = x[1]
                else:
                    setattr(v, k, x)
            return c, v

        for bad in (float("nan"), -0.1, 1.5, float("inf")):
            refused("collect_values_device", ERR_ARG, "gamma", *cv(gamma=bad)); refused("collect_values_device", ERR_ARG, "lam", *cv(lam=bad))
        refused("collect_values_device", ERR_ARG, "reserved", *cv(reserved=(0, 1))); refused("collect_values_device", ERR_ARG, "reserved", *cv(reserved=(1, 1)))
        refused("collect_values_device", ERR_ARG, "advantage", *cv(ret=None)); refused("collect_values_device", ERR_ARG, "ret", *cv(advantage=None))
        for name in ("value", "next_value", "advantage", "ret"):
            refused("collect_values_device", ERR_ARG, name, *cv(**{name: host.ctypes.data}))
            refused("collect_values_device", ERR_ARG, name, *cv(**{name: end - 8}))
        refused("collect_values_device", ERR_ARG, "value", *cv(value=None)); refused("collect_values_device", ERR_ARG, "next_value", *cv(next_value=None))
        refused("collect_values_device", ERR_ARG, "next_value", *cv(next_value=end - 4 * n_envs * (T - 1)))     # room for T - 1 decisions
        refused("collect_values_device", ERR_ARG, "n_decisions", *cv(dict(n_decisions=0)))                     # c's own errors come first
        refused("collect_values_device", ERR_ARG, "reward", *cv(dict(reward=host.ctypes.data)))
        refused("collect_values_device", ERR_STATE, "slot 2", *cv(dict(slot=2)))
        # ---- ftgp_gae_device
        def gae_args(**over):
            names = ("stream", "n_decisions", "gamma", "lam", "reward", "value", "next_value", "terminated", "truncated", "advantage", "ret")
            a = dict(zip(names, gae_ok)); a.update(over)
            return [a[k] for k in names]

        refused("gae_device", ERR_ARG, "n_decisions", *gae_args(n_decisions=0)); refused("gae_device", ERR_ARG, "n_decisions", *gae_args(n_decisions=-2))
        for bad in (float("nan"), -0.1, 1.5):
            refused("gae_device", ERR_ARG, "gamma", *gae_args(gamma=bad)); refused("gae_device", ERR_ARG, "lam", *gae_args(lam=bad))
        for name in ("reward", "value", "next_value", "terminated", "truncated", "advantage", "ret"):
            refused("gae_device", ERR_ARG, name, *gae_args(**{name: None}))
            refused("gae_device", ERR_ARG, name, *gae_args(**{name: host.ctypes.data}))
            refused("gae_device", ERR_ARG, name, *gae_args(**{name: end - 2}))
        refused("gae_device", ERR_ARG, "reward", *gae_args(n_decisions=2 ** 31 - 1))         # the T-fold size in size_t: far beyond the buffers
        # and the calls the refusals were variations of are accepted
        assert lib.fn("collect_values_device")(g.h, *cv()) == 0, lib.last_error()
        assert lib.fn("gae_device")(g.h, *gae_ok) == 0, lib.last_error()
        torch.cuda.synchronize()
        assert g.steps().max() == 1 and buf.truncated.cpu().numpy()[2].all()
        out = buf.host()
        cmod.assert_same_bits(out["value"], vm.value(vnet, out["inputs"]), "the accepted call: value")
        a, r = vm.gae(out["reward"], out["value"], out["next_value"], out["terminated"], out["truncated"], 0.9, 0.9)
        cmod.assert_same_bits(out["advantage"], a, "the accepted calls: advantage"); cmod.assert_same_bits(out["ret"], r, "the accepted calls: ret")
        # v == NULL is ftgp_collect_device
        c, _ = cv()
        assert lib.fn("collect_values_device")(g.h, c, None) == 0, lib.last_error()
        torch.cuda.synchronize()
    print("errors ok")


def vec_env(opt):
    import torch.nn as nn
    from ft_grandprix_amd.net import NetSpec, ValueSpec, value_from_torch
    from ft_grandprix_amd.vec import DeviceVecEnv, Rollout
    net = cc.driver_net(71)
    spec = NetSpec(net["layers"], **cc.fields(net))
    kw = dict(n_envs=6, n_rays=64, cars_per_env=2, roster=["agent", "nidc"], action_repeat=2, max_episode_steps=8, scan_pool=4,
              scan_max_range=3.0, state=True, spawn_mode=1, seed=9)
    a = DeviceVecEnv("small-circle", nets={0: spec}, **kw)
    b = DeviceVecEnv("small-circle", nets={0: spec}, **kw)
    a.reset(); b.reset()
    for bad in (lambda: a.collect(3, values=True), lambda: a.set_value_params(0, torch.zeros(3, device=a.device)),
                lambda: a.set_value_net(1, nn.Sequential(nn.Linear(17, 1))), lambda: a.set_value_net(0, nn.Sequential(nn.Linear(16, 1))),
                lambda: a.set_value_net(0, nn.Sequential(nn.Linear(17, 2)))):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad value-net call was accepted")
    torch.manual_seed(5)
    critic = nn.Sequential(nn.Linear(17, 32), nn.Tanh(), nn.Linear(32, 1))
    a.set_value_net(0, critic, out_scale=2.0)
    vspec = value_from_torch(critic, out_scale=2.0)
    got = a.value_net(0)
    assert got.widths == (17, 32, 1) and got.fields() == vspec.fields()
    np.testing.assert_array_equal(got.flat_params(), vspec.flat_params())
    vnet = dict(layers=vspec.layers, **vspec.fields())
    T, std, clip = 6, (0.4, 0.2), ((0.0, 3.0), (-0.4, 0.4))
    side = torch.cuda.Stream()
    roll, kept = None, None
    names = ("inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs", "value", "next_value", "advantage", "returns")
    for round_ in range(2):
        with torch.cuda.stream(side):
            gen = torch.Generator(device=a.device); gen.manual_seed(100 + round_)
            big = torch.randn((2048, 2048), generator=gen, device=a.device)
            for _ in range(20):
                big = torch.tanh(big @ big)
            noise = (torch.randn((T, 6, 1, 2), generator=gen, device=a.device) + 0.0 * big[0, 0]).contiguous()
            roll = a.collect(T, std=std, clip=clip, noise=noise, next_inputs=True, out=roll, values=True, gamma=0.97, lam=0.9)
            got = {k: getattr(roll, k).cpu().numpy() for k in names}
            plain = b.collect(T, std=std, clip=clip, noise=noise, next_inputs=True)
            want = {k: getattr(plain, k).cpu().numpy() for k in names[:7]}
        assert isinstance(roll, Rollout) and plain.value is None and plain.advantage is None
        if kept is None:
            kept = {k: getattr(roll, k).data_ptr() for k in names}
        assert kept == {k: getattr(roll, k).data_ptr() for k in names}, "out= reuses the tensors, the four new ones too"
        for k in ("value", "next_value", "advantage", "returns"):
            assert got[k].shape == (T, 6, 1) and getattr(roll, k).dtype == torch.float32
        for k in names[:7]:
            cmod.assert_same_bits(got[k].astype(F), want[k].astype(F), f"round {round_}: {k} against a plain collect")
        cmod.assert_same_bits(got["value"], vm.value(vnet, got["inputs"]), f"round {round_}: value")
        cmod.assert_same_bits(got["next_value"], vm.value(vnet, got["next_inputs"]), f"round {round_}: next_value")
        adv, ret = vm.gae(got["reward"], got["value"], got["next_value"], got["terminated"], got["truncated"], 0.97, 0.9)
        cmod.assert_same_bits(got["advantage"], adv, f"round {round_}: advantage"); cmod.assert_same_bits(got["returns"], ret, f"round {round_}: returns")
        assert torch.equal(a.obs.cpu(), b.obs.cpu()) and torch.equal(a.state.cpu(), b.state.cpu()), "obs and state after collect"
        # gae() gives the rollout's advantage again, into new tensors and into given ones; and the model's on scaled rewards
        a2, r2 = a.gae(roll.reward, roll.value, roll.next_value, roll.terminated, roll.truncated, 0.97, 0.9)
        cmod.assert_same_bits(a2.cpu().numpy(), got["advantage"], "gae(): advantage"); cmod.assert_same_bits(r2.cpu().numpy(), got["returns"], "gae(): returns")
        half = (roll.reward * 0.5).contiguous()
        a3, r3 = a.gae(half, roll.value, roll.next_value, roll.terminated, roll.truncated, 0.97, 0.9, out=(a2, r2))
        assert a3 is a2 and r3 is r2
        adv, ret = vm.gae(half.cpu().numpy(), got["value"], got["next_value"], got["terminated"], got["truncated"], 0.97, 0.9)
        cmod.assert_same_bits(a3.cpu().numpy(), adv, "gae() on scaled rewards"); cmod.assert_same_bits(r3.cpu().numpy(), ret, "gae() on scaled rewards: returns")
        # the refresh for the next round: new parameters on the current stream
        if round_ == 0:
            with torch.no_grad():
                for p in critic.parameters():
                    p.add_(0.05)
            vspec = value_from_torch(critic, out_scale=2.0)
            vnet = dict(layers=vspec.layers, **vspec.fields())
            flat = torch.from_numpy(vspec.flat_params()).to(a.device)
            a.set_value_params(0, flat)
            np.testing.assert_array_equal(a.value_net(0).flat_params(), vspec.flat_params())
    # without next_inputs the bootstrap is there all the same; out= of another kind is refused; values=False leaves None
    r4 = a.collect(3, values=True)
    assert r4.next_inputs is None and r4.next_value.shape == (3, 6, 1) and float(r4.next_value.abs().max()) > 0
    r5 = a.collect(3)
    assert r5.value is None and r5.returns is None
    for bad in (lambda: a.collect(3, values=True, out=r5), lambda: a.collect(3, values=True, gamma=1.5),
                lambda: a.gae(roll.reward, roll.value, roll.next_value, roll.terminated, roll.truncated, 0.9, 2.0),
                lambda: a.gae(roll.reward, roll.value[:3], roll.next_value, roll.terminated, roll.truncated)):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("a bad call was accepted")
    # set_net of another shape clears the value net; a ValueSpec sets one again
    wider = cc.driver_net(72, hidden=8)
    a.set_net(0, NetSpec(wider["layers"], **cc.fields(wider)))
    try:
        a.collect(3, values=True)
    except ValueError:
        pass
    else:
        raise AssertionError("collect(values=True) after set_net cleared the value net")
    a.set_value_net(0, ValueSpec(vspec.layers, **vspec.fields()))
    a.collect(3, values=True)
    a.set_value_net(0, None)
    torch.cuda.synchronize()
    a.close(); b.close()
    print("vec env ok")


SCENARIOS = {"replay_and_model": replay_and_model, "bootstrap": bootstrap, "gae": gae, "finished_and_diverged": finished_and_diverged,
             "refresh": refresh, "population": population, "rules": rules, "errors": errors, "vec_env": vec_env}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
