"""Child process of tests/test_spawn_rule.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/spawn_rule_child.py <scenario> [json options]

`model`: ftgp_reset with and without a mask under a rule, against the numpy model of the header (tests/spawn_model.py), bit for bit.
`identity`, `off`, `shards`, `errors`: a rule on one point without offsets is spawn_mode 0; NULL puts the fixed starts back; shards draw
what the whole batch draws; what must be refused.
`auto_reset`: a DeviceVecEnv with the rule (handle A) against a twin handle B on the host path that carries the same rule and is
reset(mask) where A ended, at every call, after `twin` of tests/device_contacts_child.py; the poses after every reset are the model's.
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library is loaded)

from tests import spawn_model as sp  # noqa: E402
from tests.device_twin import ContactTwin, HostTwin, _same_state, torch_driver  # noqa: E402

TRACKS = ["track", "circle", "small-circle", "inkscape"]
RULE = sp.Rule(first_point=0, n_points=100, shuffle_grid=True, margin=0.1, lateral_frac=0.8, yaw_tan=math.tan(0.1))
IDENTITY = sp.Rule(first_point=10, n_points=1, shuffle_grid=False, margin=0.0, lateral_frac=0.0, yaw_tan=0.0)
SEED = 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Model:
    """The model of a handle's rule: per track the handle's start table -- its clearances checked against the model's -- and the list of
    start points; `poses(envs, episodes)` = what those envs must spawn with."""

    def __init__(self, env, rule, seed, env_base=0):
        self.env, self.rule, self.seed, self.env_base, self.cpe = env, rule, seed, env_base, env.cars_per_env
        self.tables, self.starts, self.own_libm = [], [], True
        for k, t in enumerate(env.tracks):
            got = env.start_table(k)
            np.testing.assert_array_equal(bits(got[:, :2]), bits(np.asarray(t.path, dtype=np.float64)), err_msg=f"start table of track {k}: x, y")
            want = sp.start_table(t, poses=got)
            np.testing.assert_array_equal(bits(got[:, 4:]), bits(want[:, 4:]), err_msg=f"start table of track {k}: clearances")
            self.own_libm = self.own_libm and np.array_equal(bits(got[:, 2:4]), bits(sp.spawn_table(t)[:, 2:4]))
            self.tables.append(got)
            self.starts.append(sp.start_list(got, rule))
            assert self.starts[-1], f"track {k} has no start point"

    def poses(self, envs, episodes):
        """dict of arrays [len(envs), cars(, 4)] (tests/spawn_model.py: draw_env)."""
        rows = []
        for e in envs:
            k = int(self.env.track_of_env[e])
            rows.append(sp.draw_env(self.seed, self.env_base + int(e), int(episodes[e]), self.cpe, self.rule, self.tables[k],
                                    self.env.tracks[k].path, self.starts[k]))
        return {key: np.stack([r[key] for r in rows]) for key in rows[0]}


def check_spawned(env, model, envs, episodes, what):
    """The cars of `envs` sit where the model puts them in `episodes`, at rest, with a cleared race state."""
    cpe, envs = env.cars_per_env, np.asarray(envs)
    cars = (envs[:, None] * cpe + np.arange(cpe)[None, :]).reshape(-1)
    want = model.poses(envs, episodes)
    pose, prog = env.pose()[cars], env.progress()[cars]
    np.testing.assert_array_equal(bits(pose[:, [0, 1, 3, 6]]), bits(want["pose"].reshape(-1, 4)), err_msg=f"{what}: pose")
    assert not pose[:, [4, 5]].any() and not pose[:, 7:].any(), f"{what}: a quaternion off the yaw axis, or a velocity"
    # laps, completion, lap_completion, absolute_completion, finished, off_track, start: all 0; good_start 1; delta 0; finish_step -1
    np.testing.assert_array_equal(prog, np.tile(np.array([0, 0, 0, 0, 0, 0, 0, 1, 0, -1], dtype=np.int32), (len(cars), 1)), err_msg=f"{what}: progress")
    path = np.stack([np.asarray(env.tracks[int(env.track_of_env[e])].path, dtype=np.float64) for e in np.repeat(envs, cpe)])
    d2 = ((path[:, :, 0] - pose[:, None, 0]) ** 2 + (path[:, :, 1] - pose[:, None, 1]) ** 2)
    np.testing.assert_array_equal(d2.argmin(axis=1), want["offset"].reshape(-1), err_msg=f"{what}: offset")
    np.testing.assert_array_equal(env.centre_dist2()[cars], d2.min(axis=1), err_msg=f"{what}: centre distance")
    assert not env.steps()[envs].any() and not env.ctrl()[cars].any() and not env.lidar()[cars].any(), f"{what}: steps, ctrl or lidar"
    counts, _ = env.lap_times()
    assert not counts[cars].any()
    return want


def tally(seen, want):
    c = want["slot"].shape[1]
    seen["left"] += int((want["side"] == sp.LEFT).sum()); seen["right"] += int((want["side"] == sp.RIGHT).sum())
    seen["shuffled"] += int((want["slot"] != np.arange(c)).any(axis=1).sum()); seen["no_room"] += int((want["room"] == 0.0).sum())
    seen["moved_offset"] += int((want["offset"] != want["p"]).sum()); seen["n"] += want["p"].size


# ------------------------------------------------------------------------------------------------------------------ model
def model(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    cars, n_envs, n_rays = opt.get("cars", 3), opt.get("n_envs", 96), opt.get("n_rays", 64)
    tracks = [load_track(t) for t in TRACKS]
    lib = capi.load()
    rng = np.random.default_rng(5)
    with capi.Env(lib, tracks, n_envs=n_envs, cars_per_env=cars, n_rays=n_rays, spawn_mode=1, seed=SEED, lap_target=3) as e:
        assert not e.episodes().any()
        e.set_spawn_rule(**RULE.kwargs())
        m = Model(e, RULE, SEED)
        assert not e.episodes().any()
        ep = np.zeros(n_envs, dtype=np.int64)
        seen = dict(left=0, right=0, shuffled=0, no_room=0, moved_offset=0, n=0)
        masks = [None]
        for r in range(3):
            mask = rng.random(n_envs) < (0.5, 0.3, 0.8)[r]
            mask[[21, 85] if n_envs > 85 else [n_envs // 2, n_envs - 1]] = True       # (3 cars: env 21 straddles a wave, env 85 a workgroup of the reset kernel)
            mask[(r * 7) % n_envs] = False
            masks.append(mask)
        for r, mask in enumerate(masks):
            e.rollout("nidc", 20)                                   # a used state: steps, scans, controls, progress
            before = (e.pose(), e.progress(), e.steps(), e.lidar(), e.ctrl())
            assert before[2].all() and before[3].any()
            e.reset(None if mask is None else mask.astype(np.uint8))
            envs = np.arange(n_envs) if mask is None else np.nonzero(mask)[0]
            tally(seen, check_spawned(e, m, envs, ep, f"reset {r}"))
            ep[envs] += 1
            np.testing.assert_array_equal(e.episodes(), ep, err_msg=f"reset {r}: episodes")
            if mask is not None:                                    # the others are as they were
                keep = np.repeat(~mask, cars)
                after = (e.pose(), e.progress(), e.steps(), e.lidar(), e.ctrl())
                for x, y, per_env in zip(before, after, (0, 0, 1, 0, 0)):
                    sel = ~mask if per_env else keep
                    np.testing.assert_array_equal(x[sel], y[sel], err_msg=f"reset {r}: an env outside the mask changed")
        print(f"{cars} cars, {n_envs} envs on {len(tracks)} tracks: episodes {ep.min()} .. {ep.max()}, {seen}; quaternions of the table are "
              f"{'this' if m.own_libm else 'NOT this'} host's libm values")
        assert ep.max() >= 3 and seen["left"] > 0 and seen["right"] > 0 and seen["shuffled"] > 0 and seen["no_room"] > 0
    print("model ok")


# ------------------------------------------------------------------------------------------------------------------ identity, off, shards
def identity(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib, t = capi.load(), load_track("track")
    kw = dict(n_envs=96, cars_per_env=3, n_rays=64, spawn_mode=0, seed=SEED)
    with capi.Env(lib, t, **kw) as X, capi.Env(lib, t, **kw) as Y:
        X.set_spawn_rule(**IDENTITY.kwargs())
        X.reset(); Y.reset()
        table = X.start_table()
        np.testing.assert_array_equal(bits(X.pose()[:, [0, 1, 3, 6]]), bits(np.tile(table[[10, 12, 14], :4], (96, 1))))
        _same_state(X, Y)
        X.rollout("nidc", 50); Y.rollout("nidc", 50)
        assert X.steps().min() == 50
        _same_state(X, Y)
        mask = (np.arange(96) % 3 == 1).astype(np.uint8)
        X.reset(mask); Y.reset(mask)
        _same_state(X, Y)
        np.testing.assert_array_equal(X.episodes(), 1 + mask.astype(np.int64))
        assert not Y.episodes().any()
    print("identity ok")


def off(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib, t = capi.load(), load_track("circle")
    kw = dict(n_envs=96, cars_per_env=2, n_rays=64, spawn_mode=1, seed=SEED)
    with capi.Env(lib, t, **kw) as X, capi.Env(lib, t, **kw) as Y:
        fixed = Y.pose()
        X.set_spawn_rule(**RULE.kwargs())
        X.reset()
        assert (X.pose()[:, :2] != fixed[:, :2]).any(axis=1).mean() > 0.9 and X.episodes().min() == 1
        X.rollout("nidc", 10); Y.rollout("nidc", 10)
        X.set_spawn_rule(False)
        assert not X.episodes().any()
        X.reset(); Y.reset()
        _same_state(X, Y)
        np.testing.assert_array_equal(X.pose(), fixed)
        X.rollout("nidc", 30); Y.rollout("nidc", 30)
        mask = (np.arange(96) % 2).astype(np.uint8)
        X.reset(mask); Y.reset(mask)
        _same_state(X, Y)
        assert not X.episodes().any() and not Y.episodes().any()
    print("off ok")


def shards(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib, t = capi.load(), load_track("track")
    kw = dict(cars_per_env=3, n_rays=64, spawn_mode=1, seed=SEED)
    with capi.Env(lib, t, n_envs=8, **kw) as W, capi.Env(lib, t, n_envs=4, env_base=0, **kw) as S0, capi.Env(lib, t, n_envs=4, env_base=4, **kw) as S1:
        for h in (W, S0, S1):
            h.set_spawn_rule(**RULE.kwargs())
        m = Model(W, RULE, SEED)
        poses = []
        for r in range(2):
            for h in (W, S0, S1):
                h.reset()
            whole, parts = W.pose(), np.concatenate([S0.pose(), S1.pose()])
            np.testing.assert_array_equal(bits(whole), bits(parts), err_msg=f"reset {r}")
            np.testing.assert_array_equal(W.progress(), np.concatenate([S0.progress(), S1.progress()]))
            check_spawned(W, m, np.arange(8), np.full(8, r), f"reset {r}")
            poses.append(whole)
        assert (poses[0][:, :2] != poses[1][:, :2]).any(axis=1).all(), "the second episode starts where the first did"
        assert len({tuple(p) for p in poses[0][:, :2]}) == 24
    print("shards ok")


# ------------------------------------------------------------------------------------------------------------------ errors
def errors(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    tracks = [load_track("small-circle"), load_track("track")]
    kw = dict(n_envs=8, cars_per_env=2, n_rays=64, spawn_mode=1, seed=SEED)

    def refused(what, **fields):
        r = capi.FtgpSpawnRule(0, 100, 0, 0, 0.1, 0.5, 0.05)
        for k, v in fields.items():
            setattr(r, k, v)
        rc = lib.fn("set_spawn_rule")(E.h, r)
        assert rc == -1, f"{what}: status {rc}"
        return lib.last_error()

    with capi.Env(lib, tracks, **kw) as E, capi.Env(lib, tracks, **kw) as Y:
        E.rollout("nidc", 5); Y.rollout("nidc", 5)
        for what, fields in (("first_point -1", dict(first_point=-1)), ("first_point 100", dict(first_point=100)), ("n_points 0", dict(n_points=0)),
                             ("n_points 101", dict(n_points=101)), ("reserved set", dict(reserved=1)), ("a negative margin", dict(margin=-0.1)),
                             ("a NaN margin", dict(margin=float("nan"))), ("an infinite margin", dict(margin=float("inf"))),
                             ("a negative lateral share", dict(lateral_frac=-0.1)), ("a lateral share above 1", dict(lateral_frac=1.5)),
                             ("a NaN lateral share", dict(lateral_frac=float("nan"))), ("a negative yaw_tan", dict(yaw_tan=-1.0)),
                             ("a NaN yaw_tan", dict(yaw_tan=float("nan"))), ("an infinite yaw_tan", dict(yaw_tan=float("inf")))):
            refused(what, **fields)
        msg = refused("a margin no point keeps", margin=5.0)
        assert msg.startswith("track 0:"), msg
        # track 1 ("track") has four points without any clearance: a window of those alone leaves it, and only it, without a start point
        msg = refused("a window of blocked points", first_point=69, n_points=4, margin=0.1)
        assert msg.startswith("track 1:"), msg
        try:
            E.start_table(0)
            lib.check(lib.fn("get_start_table")(E.h, 2, np.zeros(600).ctypes.data))
        except capi.FtgpError as x:
            assert x.code == -1
        else:
            raise AssertionError("start table of track 2 of 2")
        # still usable, and without a rule
        _same_state(E, Y)
        mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
        E.reset(mask); Y.reset(mask)
        _same_state(E, Y)
        assert not E.episodes().any()
        E.rollout("nidc", 5); Y.rollout("nidc", 5)
        E.reset(); Y.reset()
        _same_state(E, Y)
        # ... and takes a good rule afterwards
        E.set_spawn_rule(**RULE.kwargs())
        E.reset()
        check_spawned(E, Model(E, RULE, SEED), np.arange(8), np.zeros(8, dtype=np.int64), "after the refusals")
    print("errors ok")


# ------------------------------------------------------------------------------------------------------------------ auto-reset
def finish_kernels_agree(track, dev):
    """Two device handles, one rule, one stream of actions: P goes through ftgp_io_finish_kernel, S -- state rows, which change no episode
    -- through ftgp_io_finish_signals_kernel.  The whole record of every car, the progress rows and the steps are equal after every
    call, and every env is reset within a few of them."""
    from ft_grandprix_amd.vec import DeviceVecEnv
    kw = dict(n_envs=8, n_rays=8, cars_per_env=3, roster=["agent", "nidc", "agent"], max_episode_steps=4, action_repeat=2, device_id=0,
              start_margin=RULE.margin, start_lateral=RULE.lateral_frac, start_yaw_jitter=0.2, shuffle_grid=True, lap_target=1,
              spawn_mode=1, seed=SEED)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    with DeviceVecEnv(track, **kw) as P, DeviceVecEnv(track, state=True, **kw) as S:
        obs = P.reset().clone()
        S.reset()
        for call in range(8):
            act = torch_driver(torch, obs, gen, dev)
            obs = P.step(act)[0].clone()
            o = S.step(act)[0].clone()
            torch.cuda.synchronize()
            at = f" through both finish kernels, call {call}"
            np.testing.assert_array_equal(o.cpu().numpy(), obs.cpu().numpy(), err_msg="obs" + at)
            np.testing.assert_array_equal(bits(S.env.snapshot()), bits(P.env.snapshot()), err_msg="snapshot" + at)
            np.testing.assert_array_equal(S.env.progress(), P.env.progress(), err_msg="progress" + at)
            np.testing.assert_array_equal(S.env.steps(), P.env.steps(), err_msg="steps" + at)
        assert P.episode_index().min() >= 3 and np.array_equal(P.episode_index(), S.episode_index()), (P.episode_index(), S.episode_index())
    print("both finish kernels: 8 calls, every env reset at least twice, records equal")


def auto_reset(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    signals = bool(opt.get("signals", False))
    n_envs, n_rays, calls = opt.get("n_envs", 96), opt.get("n_rays", 64), opt.get("calls", 24)
    roster, cpe, R, max_steps = ["agent", "nidc"], 2, 2, 6
    track = load_track("track")
    kw = dict(lap_target=1, spawn_mode=1, seed=SEED)
    sig = dict(scan_pool=4, state=True, contacts=True, terminate_on_wall_contact=True) if signals else {}
    jitter = 0.2
    lib, dev = capi.load(), torch.device("cuda", 0)
    venv = DeviceVecEnv(track, n_envs=n_envs, n_rays=n_rays, cars_per_env=cpe, roster=roster, max_episode_steps=max_steps, action_repeat=R,
                        device_id=0, start_margin=RULE.margin, start_lateral=RULE.lateral_frac, start_yaw_jitter=jitter, shuffle_grid=True,
                        **sig, **kw)
    rule = sp.Rule(0, 100, True, RULE.margin, RULE.lateral_frac, math.tan(0.5 * jitter))
    assert venv.random_start and venv.start_rule == {k: v for k, v in rule.kwargs().items()}, venv.start_rule
    A = venv.env
    B = capi.Env(lib, track, n_envs=n_envs, cars_per_env=cpe, n_rays=n_rays, **kw)
    B.set_spawn_rule(**rule.kwargs())
    m = Model(A, rule, SEED)
    paths = [np.asarray(track.path, dtype=np.float64)] * n_envs
    common = dict(pool=sig.get("scan_pool", 1), M=0.0, penalty=0.0, term_off=False, max_steps=max_steps, repeat=R, auto_reset=True)
    if signals:
        con = dict(terminate_on_wall=True, terminate_on_car=False, wall_penalty=0.0, car_penalty=0.0)
        host = ContactTwin(B, roster, paths, [track], B.envs_per_track, lib.default_vehicle(), con, **common)
    else:
        host = HostTwin(B, roster, paths, **common)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    keys = ["final_obs"] + (["state", "final_state", "contact", "final_contact"] if signals else [])
    ep = np.zeros(n_envs, dtype=np.int64)
    B.reset()
    obs = venv.reset().clone()
    torch.cuda.synchronize()
    check_spawned(A, m, np.arange(n_envs), ep, "reset()")
    ep += 1
    _same_state(A, B)
    resets, at_spawn = np.zeros(n_envs, dtype=np.int64), 0
    for call in range(calls):
        act = torch_driver(torch, obs, gen, dev)
        o, rew, te, tr, info = venv.step(act)
        got = [x.clone() for x in (o, rew, te, tr)] + [info[k].clone() for k in keys]
        torch.cuda.synchronize()
        o, rew, te, tr = [x.cpu().numpy() for x in got[:4]]
        extra = {k: x.cpu().numpy() for k, x in zip(keys, got[4:])}
        obs = got[0]
        want = host.call(act.cpu().numpy().astype(np.float64))
        at = f", call {call}"
        np.testing.assert_array_equal(te, want["terminated"], err_msg="terminated" + at)
        np.testing.assert_array_equal(tr, want["truncated"], err_msg="truncated" + at)
        np.testing.assert_array_equal(rew, want["reward"], err_msg="reward" + at)
        np.testing.assert_array_equal(o, want["obs"], err_msg="obs" + at)
        ended = want["ended"]
        if ended.any():
            np.testing.assert_array_equal(extra["final_obs"][ended], want["final_obs"], err_msg="final_obs" + at)
        if signals:
            np.testing.assert_array_equal(extra["state"], want["state"], err_msg="state" + at)
            np.testing.assert_array_equal(extra["contact"], want["contact"], err_msg="contact" + at)
            if ended.any():
                np.testing.assert_array_equal(extra["final_state"][ended], want["final_state"], err_msg="final_state" + at)
                np.testing.assert_array_equal(extra["final_contact"][ended], want["final_contact"], err_msg="final_contact" + at)
        if ended.any():
            envs = np.nonzero(ended)[0]
            check_spawned(A, m, envs, ep, "auto-reset" + at)
            at_spawn += int((A.contacts()[np.repeat(ended, cpe), 2] > 0).sum())
            ep[envs] += 1
            resets[envs] += 1
        np.testing.assert_array_equal(venv.episode_index(), ep, err_msg="episodes" + at)
        np.testing.assert_array_equal(B.episodes(), ep, err_msg="the twin's episodes" + at)
    _same_state(A, B)
    print(f"counts {host.count}; resets per env {resets.min()} .. {resets.max()}, {at_spawn} cars spawned touching a wall; kernel {A.kernel_name()}")
    assert resets.min() >= 3, resets
    venv.close()
    B.close()
    finish_kernels_agree(track, dev)
    print("auto_reset ok")


SCENARIOS = {"model": model, "identity": identity, "off": off, "shards": shards, "errors": errors, "auto_reset": auto_reset}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
