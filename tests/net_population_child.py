"""Child process of tests/test_net_population.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/net_population_child.py <scenario> [json options]

The criterion throughout is equality to the bit, no tolerance: in a handle whose slot carries a population, env e leaves exactly what
env e of a twin handle leaves -- the same config and seed, its slot holding member env_member[e]'s parameters through plain
ftgp_set_net.  M members are M twin runs, each compared on its own envs.  The plain path is held to tests/net_model.py by
tests/test_net_driver.py, so the population inherits that pin.
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
from tests import net_model as nm  # noqa: E402
from tests.net_driver_child import DRIVER, LOOP, assert_equal_state, fields, is_net_kernel, read_back, set_net  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
MAP7 = [2, 0, 0, 1, 2, 1, 0]                 # 7 envs on 3 members: not monotone, with repeats


def members(seed, M, widths=(17, 16, 2), **over):
    """M random networks of one shape (the 17-input driver of net_driver_child.py unless told otherwise) and one more, the slot's own."""
    rng = np.random.default_rng(seed)
    nets = [nm.random_net(rng, widths, **{**DRIVER, **over}) for _ in range(M + 1)]
    return nets[:M], nets[M]


def flat(net):
    return capi.net_desc(net["layers"], **fields(net))[1]


def stack(nets):
    return np.stack([flat(n) for n in nets])


def env_rows(state, envs, cpe):
    """The rows of read_back() that belong to the envs `envs`: a row per car, but for `steps`, a row per env."""
    cars = (np.asarray(envs)[:, None] * cpe + np.arange(cpe)[None, :]).ravel()
    return {k: v[envs] if k == "steps" else v[cars] for k, v in state.items()}


def compare_with_twins(make, prepare, nets, own, env_member, run, what, slot=0):
    """`make()` a handle, `prepare` it (the slot's own network `own` is set first), give slot `slot` the population and `run` it; then per
    member a twin with that member's parameters through ftgp_set_net, compared on the member's envs."""
    M = len(nets)
    with make() as g:
        set_net(g, slot, own)
        prepare(g)
        g.set_net_population(slot, stack(nets), env_member)
        n, m = g.get_net_population(slot)
        want_map = np.arange(g.n_envs) % M if env_member is None else np.asarray(env_member)
        assert n == M
        np.testing.assert_array_equal(m, want_map)
        run(g)
        got, name, cpe = read_back(g), g.kernel_name(), g.n_cars // g.n_envs
    assert is_net_kernel(name), name
    seen = 0
    for k in range(M):
        envs = np.flatnonzero(want_map == k)
        if envs.size == 0:
            continue
        with make() as twin:
            set_net(twin, slot, nets[k])
            prepare(twin)
            run(twin)
            assert_equal_state(env_rows(got, envs, cpe), env_rows(read_back(twin), envs, cpe), f"{what}: member {k}, envs {envs.tolist()}")
            others = np.flatnonzero(want_map != k)
            if others.size:          # the members do differ: a population that ran one member everywhere would not pass
                assert not np.array_equal(env_rows(got, others, cpe)["pose"], env_rows(read_back(twin), others, cpe)["pose"]), (what, k)
        seen += envs.size
    assert seen == len(want_map)
    return got


def rollout(opt):
    if opt.get("cpb"):
        os.environ["FTGP_CARS_PER_BLOCK"], os.environ["FTGP_VERBOSE"] = str(opt["cpb"]), "1"
    lib = capi.load()
    t = load_track("small-circle")
    nets, own = members(11, 3)
    for env_member in (MAP7, None):
        got = compare_with_twins(lambda: capi.Env(lib, t, n_envs=7, **LOOP), lambda g: None, nets, own, env_member,
                                 lambda g: g.rollout("net0", 40), f"rollout, map {env_member}")
        assert np.abs(got["pose"][:, 7:9]).max() > 0.1, "the cars did not move"
    print("rollout ok")


def shapes(opt):
    lib = capi.load()
    t = load_track("small-circle")
    # a hidden layer of 65 .. 128 neurons: the WIDE rows, ld = 128; count = 17*100 + 100 + 2*100 + 2 = 2002, no multiple of 64
    nets, own = members(21, 3, widths=(17, 100, 2))
    assert flat(nets[0]).size == 2002
    compare_with_twins(lambda: capi.Env(lib, t, n_envs=7, **LOOP), lambda g: None, nets, own, MAP7, lambda g: g.rollout("net0", 25), "wide hidden layer")
    # more than 64 inputs: the second input register.  512 rays of pool 4, beams 16 .. 95 and the state: 85 inputs, two hidden layers
    nets, own = members(22, 3, widths=(85, 33, 16, 2), beam_first=16)
    compare_with_twins(lambda: capi.Env(lib, t, n_envs=7, n_rays=512, spawn_mode=1, seed=5), lambda g: None, nets, own, MAP7,
                       lambda g: g.rollout("net2", 25), "85 inputs", slot=2)
    print("shapes ok")


def roster(opt):
    lib = capi.load()
    names = ["net0", "net1", "fast", "nidc"]
    nets, own = members(31, 3, widths=(17 + 4 + 8 * 2, 16, 2))
    other = members(32, 1)[0][0]
    rivals = dict(rivals=True, n_rivals=2, n_beams=12)         # (random_net counted the rival entries as beams)

    def prepare(g):
        set_net(g, 1, other)
        g.set_car_policies(names)
    for what, tracks, kw in (("one track", load_track("small-circle"), dict(n_envs=7)),
                             ("two tracks", [load_track("small-circle"), load_track("circle")], dict(n_envs=7, envs_per_track=(3, 4)))):
        compare_with_twins(lambda: capi.Env(lib, tracks, cars_per_env=4, **kw, **LOOP), prepare, [dict(n, **rivals) for n in nets], dict(own, **rivals), MAP7,
                           lambda g: g.rollout("per_car", 30), f"roster, {what}")
    print("roster ok")


def device_setter(opt):
    lib = capi.load()
    t = load_track("small-circle")
    first, own = members(41, 3)
    second, _ = members(42, 3)
    map2 = [1, 1, 2, 0, 0, 2, 1]
    side = torch.cuda.Stream()
    with capi.Env(lib, t, n_envs=7, **LOOP) as g, capi.Env(lib, t, n_envs=7, **LOOP) as h:
        for e in (g, h):
            set_net(e, 0, own)
            e.set_net_population(0, stack(first), MAP7)
            e.rollout("net0", 10)
        # parameters and map replaced between two launches from torch tensors produced on a stream of their own
        with torch.cuda.stream(side):
            p = torch.from_numpy(stack(second)).to("cuda") + 0.0
            m = torch.tensor(map2, dtype=torch.int32, device="cuda")
            g.set_net_population_device(0, p.data_ptr(), m.data_ptr(), side.cuda_stream)
        g.rollout("net0", 10)
        h.set_net_population(0, stack(second), map2)
        h.rollout("net0", 10)
        assert_equal_state(read_back(g), read_back(h), "device setter against the host setter")
        for e in (g, h):
            n, mm = e.get_net_population(0)
            assert n == 3
            np.testing.assert_array_equal(mm, map2)
            for k in range(3):
                np.testing.assert_array_equal(e.get_net_population(0, k), flat(second[k]), err_msg=f"member {k}")
        np.testing.assert_array_equal(np.concatenate([np.concatenate([W.ravel(), b]) for W, b in g.net(0)[1]]), flat(own), err_msg="ftgp_get_net keeps the slot's single set")
        # the map alone, with entries out of range: member 0
        bad = torch.tensor([0, 3, -1, 2, 1, 7, 2], dtype=torch.int32, device="cuda")
        g.set_net_population_device(0, 0, bad.data_ptr(), torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(g.get_net_population(0)[1], [0, 0, 0, 2, 1, 0, 2])
        # the parameters alone keep the map; the same tensors again leave the padding zero -- as far as an evaluation shows it: equal to
        # the host setter's, and with every weight and bias shrunk to zero act(0) scaled and offset whatever the inputs
        g.set_net_population_device(0, p.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        g.set_net_population_device(0, p.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(g.get_net_population(0)[1], [0, 0, 0, 2, 1, 0, 2])
        h.set_net_population(0, stack(second), [0, 0, 0, 2, 1, 0, 2])
        rng = np.random.default_rng(4)
        scans = nm.eval_scans(rng, g.n_cars, 64, own["max_range"])
        ctrl = g.ctrl()
        h.set_pose(g.pose()); h.set_ctrl(ctrl)
        np.testing.assert_array_equal(g.policy_eval("net0", scans), h.policy_eval("net0", scans))
        zero = torch.zeros_like(p)
        g.set_net_population_device(0, zero.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        h.set_net_population(0, np.zeros_like(stack(second)), [0, 0, 0, 2, 1, 0, 2])
        g.set_ctrl(ctrl); h.set_ctrl(ctrl)
        ug, uh = g.policy_eval("net0", scans), h.policy_eval("net0", scans)
        np.testing.assert_array_equal(ug, uh)
        np.testing.assert_array_equal(ug, np.broadcast_to(np.array([1.5, 0.0]), ug.shape))     # tanh(0) * scale + offset
        # refusals of the device setter: a host pointer, a slot without a population, a slot not defined
        host = np.zeros(4000, dtype=np.float32)
        fn = lib.fn("set_net_population_device")
        assert fn(g.h, None, 0, host.ctypes.data, None) == ERR_ARG and "ftgp_set_net_population_device" in lib.last_error()
        assert fn(g.h, None, 0, None, host.ctypes.data) == ERR_ARG and "env_member" in lib.last_error()
        assert fn(g.h, None, 1, p.data_ptr(), None) == ERR_STATE and fn(g.h, None, 4, p.data_ptr(), None) == ERR_ARG
        set_net(g, 1, own)
        assert fn(g.h, None, 1, p.data_ptr(), None) == ERR_STATE and "population" in lib.last_error()
        g.set_ctrl(ctrl)
        np.testing.assert_array_equal(g.policy_eval("net0", scans), ug)
    # more members than the grid of the conversion kernel has rows (1024): its threads walk the members
    M = 1100
    with capi.Env(lib, t, n_envs=M, **LOOP) as g:
        set_net(g, 0, own)
        rows = np.random.default_rng(43).standard_normal((M, flat(own).size)).astype(np.float32)
        g.set_net_population(0, np.zeros_like(rows))
        p = torch.from_numpy(rows).to("cuda")
        g.set_net_population_device(0, p.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        for k in (0, 1, 1023, 1024, 1025, M - 1):
            np.testing.assert_array_equal(g.get_net_population(0, k), rows[k], err_msg=f"member {k} of {M}")
    print("device setter ok")


def policy_eval(opt):
    lib = capi.load()
    t = load_track("small-circle")
    nets, own = members(51, 3)
    rng = np.random.default_rng(5)
    with capi.Env(lib, t, n_envs=7, cars_per_env=2, **LOOP) as g, capi.Env(lib, t, n_envs=7, cars_per_env=2, **LOOP) as twin:
        pose, ctrl = nm.eval_records(rng, g.n_cars)
        pose[:, :3] = g.pose()[:, :3]
        scans = nm.eval_scans(rng, g.n_cars, 64, own["max_range"])
        set_net(g, 0, own)
        g.set_net_population(0, stack(nets), MAP7)
        g.set_pose(pose); g.set_ctrl(ctrl)
        got = g.policy_eval("net0", scans)
        for k in range(3):
            set_net(twin, 0, nets[k])
            twin.set_pose(pose); twin.set_ctrl(ctrl)
            want = twin.policy_eval("net0", scans)
            np.testing.assert_array_equal(want, nm.evaluate(nets[k], scans, twin.pose(), ctrl))        # (the plain path's pin)
            cars = np.flatnonzero(np.repeat(np.asarray(MAP7) == k, 2))
            np.testing.assert_array_equal(got[cars], want[cars], err_msg=f"policy_eval, member {k}")
        assert np.abs(got).max() > 0
    print("policy_eval ok")


def collect(opt):
    from ft_grandprix_amd import net
    from ft_grandprix_amd.vec import DeviceVecEnv
    nets, own = members(61, 3)
    specs = [net.NetSpec(n["layers"], **fields(n)) for n in nets]
    kw = dict(n_envs=7, n_rays=64, cars_per_env=2, roster=["agent", "nidc"], action_repeat=2, max_episode_steps=6, scan_pool=4,
              scan_max_range=3.0, state=True, spawn_mode=1, seed=9)
    T, std, clip = 8, (0.4, 0.2), ((0.0, 3.0), (-0.4, 0.4))
    names = ("inputs", "mean", "action", "reward", "terminated", "truncated", "next_inputs")

    def run(env):
        env.reset()
        gen = torch.Generator(device=env.device); gen.manual_seed(7)
        noise = torch.randn((T, 7, 1, 2), generator=gen, device=env.device)
        roll = env.collect(T, slot=0, std=std, clip=clip, noise=noise, next_inputs=True)
        return {k: getattr(roll, k).cpu().numpy() for k in names}, env.env.pose()
    a = DeviceVecEnv("small-circle", nets={0: net.NetSpec(own["layers"], **fields(own))}, **kw)
    a.set_population(0, net.stack_params(specs), np.asarray(MAP7))
    n, m, params = a.population(0)
    assert n == 3
    np.testing.assert_array_equal(m, MAP7)
    np.testing.assert_array_equal(params, net.stack_params(specs))
    got, pose = run(a)
    assert int((got["terminated"] | got["truncated"]).sum()) >= 7, "no auto-reset happened"
    # the device way: the same members, shuffled, from tensors on the env's device; then back
    p = torch.from_numpy(net.stack_params(specs[::-1])).to(a.device)
    m = torch.tensor([2 - k for k in MAP7], dtype=torch.int32, device=a.device)
    a.set_population(0, p, m)
    again, pose_again = run(a)
    # env_member="keep" leaves the map in force, None is e % n_members on the device way too
    a.set_population(0, p, "keep")
    np.testing.assert_array_equal(a.population(0)[1], [2 - k for k in MAP7])
    a.set_population(0, p)
    np.testing.assert_array_equal(a.population(0)[1], np.arange(7) % 3)
    a.set_population(0, p.cpu().numpy(), "keep")
    np.testing.assert_array_equal(a.population(0)[1], np.arange(7) % 3)
    a.close()
    for k in range(3):
        b = DeviceVecEnv("small-circle", nets={0: specs[k]}, **kw)
        want, pose_b = run(b)
        b.close()
        envs = np.flatnonzero(np.asarray(MAP7) == k)
        for name in names:
            for g, what in ((got, "host way"), (again, "device way")):
                np.testing.assert_array_equal(g[name][:, envs].view(np.uint8), want[name][:, envs].view(np.uint8), err_msg=f"collect, {what}, member {k}: {name}")
        cars = np.flatnonzero(np.repeat(np.asarray(MAP7) == k, 2))
        np.testing.assert_array_equal(pose[cars], pose_b[cars]); np.testing.assert_array_equal(pose_again[cars], pose_b[cars])
    print("collect ok")


def env_states(opt):
    from ft_grandprix_amd import net
    from ft_grandprix_amd.vec import DeviceVecEnv
    nets, own = members(71, 3)
    specs = [net.NetSpec(n["layers"], **fields(n)) for n in nets]
    kw = dict(n_envs=7, n_rays=64, cars_per_env=2, roster=["agent", "net0"], action_repeat=1, scan_pool=4, scan_max_range=3.0, state=True,
              spawn_mode=1, seed=9)

    def run(env, after_fork=lambda: None):
        """five calls, then env 0's state into every env, then fifteen calls: each env follows its own member from env 0's state"""
        env.reset()
        act = torch.tensor([1.5, 0.1], device=env.device).expand(7, 1, 2).contiguous()
        for _ in range(5):
            env.step(act)
        env.fork(torch.zeros(7, dtype=torch.int64, device=env.device))
        start = env.env.pose().copy()
        after_fork()
        for _ in range(15):
            env.step(act)
        return start, read_back(env.env)
    a = DeviceVecEnv("small-circle", nets={0: net.NetSpec(own["layers"], **fields(own))}, **kw)
    a.set_population(0, net.stack_params(specs), np.asarray(MAP7))
    start, got = run(a)
    np.testing.assert_array_equal(a.env.get_net_population(0)[1], MAP7)
    assert is_net_kernel(a.env.kernel_name())
    a.close()
    for e in range(1, 7):
        np.testing.assert_array_equal(start[2 * e:2 * e + 2, 3:], start[0:2, 3:], err_msg="every env starts from env 0's state")
    assert not np.array_equal(got["pose"][0:2], got["pose"][2:4]), "envs of different members part ways"
    for k in range(3):
        # the twin reaches env 0's state as the population's env 0 did, under env 0's member, and holds member k from the fork on
        b = DeviceVecEnv("small-circle", nets={0: specs[MAP7[0]]}, **kw)
        start_b, want = run(b, lambda: b.set_net(0, specs[k]))
        b.close()
        np.testing.assert_array_equal(start_b, start)
        envs = np.flatnonzero(np.asarray(MAP7) == k)
        assert_equal_state(env_rows(got, envs, 2), env_rows(want, envs, 2), f"fork, member {k}")
    print("env states ok")


def removal(opt):
    lib = capi.load()
    t = load_track("small-circle")
    nets, own = members(81, 3)
    with capi.Env(lib, t, n_envs=7, **LOOP) as g, capi.Env(lib, t, n_envs=7, **LOOP) as fresh:
        set_net(g, 0, own); set_net(fresh, 0, own)
        g.set_net_population(0, stack(nets), MAP7)
        g.set_net_population(0, None)
        assert g.get_net_population(0) == (0, None)
        for e in (g, fresh):
            e.rollout("net0", 30)
        assert_equal_state(read_back(g), read_back(fresh), "n_members = 0 restores the single set")
        # reset leaves a population alone; ftgp_set_net defines the slot without one
        g.set_net_population(0, stack(nets), MAP7)
        g.reset()
        assert g.get_net_population(0)[0] == 3
        set_net(g, 0, own)
        assert g.get_net_population(0) == (0, None)
        g.reset(); fresh.reset()
        for e in (g, fresh):
            e.rollout("net0", 30)
        assert_equal_state(read_back(g), read_back(fresh), "ftgp_set_net removes the population")
        # a launch that names no network runs what it ran, population or not
        g.set_net_population(0, stack(nets), MAP7)
        for e in (g, fresh):
            e.rollout("fast", 20)
        assert g.kernel_name() == fresh.kernel_name() and not is_net_kernel(g.kernel_name()), g.kernel_name()
        assert_equal_state(read_back(g), read_back(fresh), "rollout fast beside a population")
    print("removal ok")


def errors(opt):
    lib = capi.load()
    t = load_track("small-circle")
    nets, own = members(91, 3)
    rng = np.random.default_rng(4)
    fn = lib.fn("set_net_population")
    with capi.Env(lib, t, n_envs=7, **LOOP) as g:
        scans = nm.eval_scans(rng, g.n_cars, 64, own["max_range"])
        params = stack(nets)
        good = np.asarray(MAP7, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
        assert fn(g.h, 0, 3, ptr(params), ptr(good)) == ERR_STATE and "not defined" in lib.last_error()
        assert lib.fn("get_net_population")(g.h, 0, None, None, 0, None) == ERR_STATE
        set_net(g, 0, own)
        g.set_ctrl(np.zeros((g.n_cars, 2)))
        single = g.policy_eval("net0", scans)

        def in_force(want, what):
            g.set_ctrl(np.zeros((g.n_cars, 2)))
            np.testing.assert_array_equal(g.policy_eval("net0", scans), want, err_msg=f"the slot after {what}")

        def refused(expect, word, slot=0, n=3, p=params, m=good):
            rc = fn(g.h, slot, n, ptr(p), ptr(m))
            assert rc == expect and word in lib.last_error(), (rc, word, lib.last_error())
        for stage, want in (("without a population", single), ("with one", None)):
            if want is None:
                g.set_net_population(0, params, MAP7)
                g.set_ctrl(np.zeros((g.n_cars, 2)))
                want = g.policy_eval("net0", scans)
                assert not np.array_equal(want, single)
            refused(ERR_ARG, "slot", slot=-1); refused(ERR_ARG, "slot", slot=4); refused(ERR_STATE, "not defined", slot=3)
            refused(ERR_ARG, "n_members", n=-1); refused(ERR_ARG, "n_members", n=8)
            refused(ERR_ARG, "params", p=None)
            for k, v in ((0, 3), (6, -1), (3, 2 ** 31 - 1)):
                bad = good.copy(); bad[k] = v
                refused(ERR_ARG, f"env_member[{k}]", m=bad)
            in_force(want, f"the refusals {stage}")
            n_out = capi.C.c_int32(-1)
            assert lib.fn("get_net_population")(g.h, 0, capi.C.byref(n_out), None, 0, None) == 0 and n_out.value == (0 if stage.startswith("without") else 3)
        # ftgp_set_net_device on a slot with a population; ftgp_get_net_population's own refusals
        p = torch.from_numpy(flat(own)).to("cuda")
        assert lib.fn("set_net_device")(g.h, None, 0, p.data_ptr()) == ERR_STATE and "ftgp_set_net_population_device" in lib.last_error()
        out = np.zeros(params.shape[1], dtype=np.float32)
        get = lib.fn("get_net_population")
        assert get(g.h, 0, None, None, 3, out.ctypes.data) == ERR_ARG and "member" in lib.last_error()
        assert get(g.h, 0, None, None, -1, out.ctypes.data) == ERR_ARG and get(g.h, 5, None, None, 0, None) == ERR_ARG
        in_force(want, "ftgp_set_net_device's refusal")
    print("errors ok")


SCENARIOS = {"rollout": rollout, "shapes": shapes, "roster": roster, "device_setter": device_setter, "policy_eval": policy_eval, "collect": collect,
             "env_states": env_states, "removal": removal, "errors": errors}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
