"""Child process of tests/test_multitrack.py: one GPU scenario per process (torch, when used, imported before libftgp.so is loaded: see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held.

    python tests/multitrack_child.py <scenario> [json options]

Every scenario checks a multi-track handle (ftgp_create_tracks) against one single-track handle per env block t, created with
track = tracks[t], n_envs = envs_per_track[t] and env_base = env_base + first_t: bit for bit.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ["track", "circle", "small-circle", "inkscape"]
COUNTS = (37, 64, 5, 150)


def firsts(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int)


def state(env):
    counts, ring = env.lap_times()
    return {"lidar": env.lidar(), "pose": env.pose(), "progress": env.progress(), "race_steps": env.race_steps(), "lap_counts": counts,
            "lap_ring": ring, "winners": env.winners(), "steps": env.steps(), "ctrl": env.ctrl()}


def compare(multi, singles, counts, cpe, what):
    m = state(multi)
    for t, (single, first, n) in enumerate(zip(singles, firsts(counts), counts)):
        s = state(single)
        for k, v in s.items():
            lo, hi = (first, first + n) if k in ("winners", "steps") else (first * cpe, (first + n) * cpe)
            np.testing.assert_array_equal(m[k][lo:hi], v, err_msg=f"{what}: block {t}, {k}")


def handles(lib, tracks, counts, **kw):
    from ft_grandprix_amd import capi
    env_base = kw.pop("env_base", 0)
    multi = capi.Env(lib, tracks, n_envs=int(sum(counts)), envs_per_track=counts, env_base=env_base, **kw)
    singles = [capi.Env(lib, t, n_envs=int(n), env_base=env_base + int(f), **kw) for t, n, f in zip(tracks, counts, firsts(counts))]
    return multi, singles


def teleport(multi, singles, tracks, counts, cpe, spawn_mode, env_base, ahead):
    """Every car to the centre-line point `ahead` past its spawn point, on its own track (ftgp_set_pose + ftgp_eval_progress)."""
    pose = multi.pose()
    for t, (track, first, n) in enumerate(zip(tracks, firsts(counts), counts)):
        path = np.asarray(track.path, dtype=np.float64)
        for e in range(first, first + n):
            for c in range(cpe):
                p = (c + 5) * 2 if spawn_mode == 0 else (10 + 7 * (env_base + e) + 2 * c) % 98
                q = (p + ahead) % 100
                a = np.arctan2(path[(q + 1) % 100, 1] - path[q, 1], path[(q + 1) % 100, 0] - path[q, 0])
                row = pose[e * cpe + c]
                row[0], row[1], row[3], row[6] = path[q, 0], path[q, 1], np.cos(a / 2), np.sin(a / 2)
    multi.set_pose(pose)
    multi.eval_progress()
    for s, first, n in zip(singles, firsts(counts), counts):
        s.set_pose(pose[first * cpe:(first + n) * cpe])
        s.eval_progress()


def equivalence(opt):
    """The matrix of one shape (cars_per_env, n_rays, lidar_mode), both spawn modes, five policies: rollouts, a masked reset across
    blocks, set_pose + eval_progress and a drive over the line; every read-back and the metrics record."""
    from ft_grandprix_amd import capi, dist
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    cpe, R, mode = opt["cars_per_env"], opt["n_rays"], opt["lidar_mode"]
    steps = opt.get("steps", 200)
    tracks = [load_track(n) for n in NAMES]
    roster = (["nidc", "fast", "random"] * 3)[:cpe] if cpe > 1 else ["fast"]
    for spawn_mode, env_base in ((0, 0), (1, 11)):
        kw = dict(cars_per_env=cpe, n_rays=R, lidar_mode=mode, spawn_mode=spawn_mode, env_base=env_base, seed=99, lap_target=1)
        multi, singles = handles(lib, tracks, COUNTS, **kw)
        compare(multi, singles, COUNTS, cpe, "after create")
        for policy in ("fast", "nidc", "random", "per_car", "host"):
            what = f"cpe {cpe} rays {R} {mode} spawn {spawn_mode} env_base {env_base} {policy}"
            envs = [multi] + singles
            for e in envs:
                e.reset()
            if policy == "per_car":
                for e in envs:
                    e.set_car_policies(roster)
            if policy == "host":
                rng = np.random.default_rng(5)
                ctrl = np.stack([rng.uniform(0.5, 2.0, multi.n_cars), rng.uniform(-0.3, 0.3, multi.n_cars)], axis=1)
                multi.set_ctrl(ctrl)
                for s, f, n in zip(singles, firsts(COUNTS), COUNTS):
                    s.set_ctrl(ctrl[f * cpe:(f + n) * cpe])
                for e in envs:
                    e.step(steps)
            else:
                for e in envs:
                    e.rollout(policy, steps)
            compare(multi, singles, COUNTS, cpe, what + ": rollout")
            # the launch's metrics record = the per-block records combined as shards are
            got = dist.reduce_metrics(multi.metrics_local())
            want = dist.reduce_metrics(np.stack([s.metrics_local() for s in singles]))
            got.pop("ranks"), want.pop("ranks")
            assert got == want, (what, got, want)
            mask = (np.arange(multi.n_envs) % 3 == 1).astype(np.uint8)
            multi.reset(mask)
            for s, f, n in zip(singles, firsts(COUNTS), COUNTS):
                s.reset(mask[f:f + n])
            compare(multi, singles, COUNTS, cpe, what + ": masked reset")
            teleport(multi, singles, tracks, COUNTS, cpe, spawn_mode, env_base, 97)
            compare(multi, singles, COUNTS, cpe, what + ": set_pose + eval_progress")
            for e in envs:
                if policy == "host":
                    e.step(steps // 2)
                else:
                    e.rollout(policy, steps // 2)
            compare(multi, singles, COUNTS, cpe, what + ": over the line")
            got = multi.metrics_local()
            want = dist.reduce_metrics(np.stack([s.metrics_local() for s in singles]))
            g = dist.reduce_metrics(got)
            g.pop("ranks"), want.pop("ranks")
            assert g == want, (what, g, want)
        print(f"equivalence ok: cpe {cpe} rays {R} {mode} spawn {spawn_mode}, laps {int(multi.progress()[:, 0].sum())}, "
              f"finished {int(multi.progress()[:, 4].sum())}, kernel {multi.kernel_name()}")
        for e in [multi] + singles:
            e.close()


def oracle_blocks(opt):
    """A small four-track handle against the CPU oracle run block by block with env_base."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from tests.helpers import load_oracle
    lib, ora = capi.load(), load_oracle()
    tracks = [load_track(n) for n in NAMES]
    counts, base = (3, 2, 1, 2), 5
    kw = dict(n_rays=36, spawn_mode=1, seed=7)
    with capi.Env(lib, tracks, n_envs=sum(counts), envs_per_track=counts, env_base=base, **kw) as g:
        g.rollout("nidc", 50)
        for t, f, n in zip(tracks, firsts(counts), counts):
            with capi.Env(ora, t, n_envs=n, env_base=base + int(f), **kw) as o:
                o.rollout("nidc", 50)
                np.testing.assert_array_equal(g.lidar()[f:f + n], o.lidar())
                np.testing.assert_array_equal(g.progress()[f:f + n], o.progress())
                np.testing.assert_allclose(g.pose()[f:f + n], o.pose(), rtol=0, atol=1e-9)
    print("oracle ok")


def one_track(opt):
    """ftgp_create_tracks with one track is ftgp_create."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    t = load_track("small-circle")
    kw = dict(n_envs=300, n_rays=1080, spawn_mode=1, seed=3, env_base=4)
    with capi.Env(lib, [t], **kw) as a, capi.Env(lib, t, **kw) as b:
        assert a.kernel_name() == b.kernel_name()
        for e in (a, b):
            e.rollout("fast", 300)
        for k, v in state(b).items():
            np.testing.assert_array_equal(state(a)[k], v, err_msg=k)
        np.testing.assert_array_equal(a.metrics_local(), b.metrics_local())
    print("one track ok")


def orders(opt):
    """FTGP_TRACK_ORDER=blocks and =xcd give identical results."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    tracks = [load_track(n) for n in NAMES]
    out = []
    for order in ("blocks", "xcd"):
        os.environ["FTGP_TRACK_ORDER"] = order
        with capi.Env(lib, tracks, n_envs=sum(COUNTS), envs_per_track=COUNTS, n_rays=1080, cars_per_env=3, spawn_mode=1, seed=1) as e:
            e.rollout("fast", 300)
            out.append((state(e), e.metrics_local()))
    for k, v in out[0][0].items():
        np.testing.assert_array_equal(out[1][0][k], v, err_msg=k)
    np.testing.assert_array_equal(out[0][1], out[1][1])
    print("orders ok")


def distance_fields(opt):
    """get_distance_field(t) is the single-track field; fixture G8 (all four tracks) through ONE four-track handle."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from tests.helpers import golden
    lib = capi.load()
    tracks = [load_track(n) for n in NAMES]
    g = np.load(golden("g8_fakelidar_step.npz"))
    counts = tuple(len(g[f"{n}_xy"]) for n in NAMES)
    for R in (36, 1080):
        with capi.Env(lib, tracks, n_envs=sum(counts), envs_per_track=counts, n_rays=R, lidar_mode="fakelidar", fan_dirs=g[f"fan_{R}"]) as e:
            if R == 36:
                for k, t in enumerate(tracks):
                    with capi.Env(lib, t, n_envs=1, n_rays=R, lidar_mode="fakelidar") as s:
                        np.testing.assert_array_equal(e.get_distance_field(k), s.distance_field())
                try:
                    e.distance_field()
                except capi.FtgpError as x:
                    assert x.code == -4, x
                else:
                    raise AssertionError("ftgp_get_distance_field answered on a four-track handle")
            pose = e.pose()
            xy = np.concatenate([g[f"{n}_xy"] for n in NAMES])
            quat = np.concatenate([g[f"{n}_quat"] for n in NAMES])
            pose[:, 0:2] = xy
            pose[:, 3], pose[:, 6] = quat[:, 0], quat[:, 1]
            pose[:, 7:] = 0.0
            e.set_pose(pose)
            e.step(1)
            got = e.lidar()
            for n, f, c in zip(NAMES, firsts(counts), counts):
                np.testing.assert_array_equal(got[f:f + c], g[f"{n}_{R}_ranges"], err_msg=f"{n} {R}")
    print("distance fields ok")


def comm_refused(opt):
    """ftgp_comm_init on a handle with more than one track: FTGP_ERR_STATE (before RCCL is touched)."""
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    with capi.Env(lib, [load_track("circle"), load_track("track")], n_envs=4, n_rays=64) as e:
        try:
            e.comm_init(bytes(128), 0, 1)
        except capi.FtgpError as x:
            assert x.code == -4 and "multi-track" in str(x), x
        else:
            raise AssertionError("ftgp_comm_init accepted a multi-track handle")
    print("comm refused ok")


def device_io(opt):
    """ftgp_step_device / DeviceVecEnv on four tracks against the per-block envs, every call: obs, reward, terminated, truncated,
    final_obs; auto-resets in every block; track_index."""
    import torch
    from ft_grandprix_amd.vec import DeviceVecEnv
    dev = torch.device("cuda", 0)
    roster, M, AR, calls = ["agent", "fast"], opt.get("max_episode_steps", 120), opt.get("action_repeat", 1), opt.get("calls", 400)
    kw = dict(n_rays=1080, cars_per_env=2, roster=roster, max_episode_steps=M, action_repeat=AR, spawn_mode=1, seed=5, lap_target=1)
    multi = DeviceVecEnv(NAMES, n_envs=sum(COUNTS), envs_per_track=COUNTS, env_base=3, **kw)
    singles = [DeviceVecEnv(n, n_envs=c, env_base=3 + int(f), **kw) for n, c, f in zip(NAMES, COUNTS, firsts(COUNTS))]
    want_index = torch.repeat_interleave(torch.arange(4), torch.tensor(COUNTS)).to(dev)
    assert multi.track_index.dtype == torch.int64 and multi.track_index.device == dev and torch.equal(multi.track_index, want_index)
    assert multi.env.kernel_name().endswith(", true>")
    for v in [multi] + singles:
        v.reset()
    g = torch.Generator(device=dev).manual_seed(11)
    n_term = n_trunc = 0
    ended_blocks = set()
    for call in range(calls):
        act = torch.stack([torch.rand((multi.n_envs, 1), device=dev, generator=g) * 3.0,
                           torch.rand((multi.n_envs, 1), device=dev, generator=g) * 0.6 - 0.3], dim=-1).contiguous()
        mo = [x.clone() for x in multi.step(act)[:4]] + [multi.final_obs.clone()]
        so = []
        for s, f, c in zip(singles, firsts(COUNTS), COUNTS):
            r = s.step(act[f:f + c].contiguous())
            so.append([x.clone() for x in r[:4]] + [s.final_obs.clone()])
        for k, name in enumerate(("obs", "reward", "terminated", "truncated", "final_obs")):
            # (final_obs whole: rows of envs that did not end hold older values, the same on both sides when every call matched)
            np.testing.assert_array_equal(mo[k].cpu().numpy(), torch.cat([b[k] for b in so]).cpu().numpy(), err_msg=f"call {call} {name}")
        n_term += int(mo[2].sum()); n_trunc += int(mo[3].sum())
        ended_blocks |= set(multi.track_index[(mo[2] | mo[3])].tolist())
    assert ended_blocks == {0, 1, 2, 3}, f"auto-resets in blocks {sorted(ended_blocks)} only"
    torch.cuda.synchronize()
    print(f"device io ok: {calls} calls, {n_term} terminations, {n_trunc} truncations, auto-resets in blocks {sorted(ended_blocks)}")
    for v in [multi] + singles:
        v.close()


SCENARIOS = {"equivalence": equivalence, "oracle_blocks": oracle_blocks, "one_track": one_track, "orders": orders,
             "distance_fields": distance_fields, "comm_refused": comm_refused, "device_io": device_io}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
