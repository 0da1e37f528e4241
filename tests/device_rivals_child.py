"""Child process of tests/test_device_rivals.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/device_rivals_child.py <scenario> [json options]

`set_poses`: poses and velocities put with set_pose + eval_progress; ftgp_get_rivals and ftgp_rivals_device against the numpy model of
the header (tests/rival_model.py), bit for bit.
`finished`: finishers made by teleport: ghosts to the others, their place the one of ftgp_get_winners.
`closed_loop`: a DeviceVecEnv with every signal on against the model at the records read back at every call, with a twin without
rivals, a twin without the place reward and a twin without auto-reset (the records before a reset).
`multi_track`, `off`: rows follow each env's own path; rivals off is the old call, and what must be refused.
"""
import ctypes
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library is loaded)

from tests import frame_model as fm  # noqa: E402
from tests import rival_model as rm  # noqa: E402
from tests.device_twin import refused  # noqa: E402
from tests.helpers import open_field  # noqa: E402

DEV = "cuda:0"
STATE, ARG = -4, -1          # FTGP_ERR_STATE, FTGP_ERR_ARG
SHAPES = ((1, 1), (7, 1), (3, 3), (4, 8), (11, 3), (13, 5), (87, 3))          # (n_envs, cars_per_env): 1, 7, 9, 32, 33, 65 and 261 cars
SLOTS = (0, 1, 3, 7)
SQUARE_SHIFT = np.array([8.0, -24.0])          # dyadic: the hand-written envs stay exact


def square_track():
    """`square_path` of tests/frame_model.py, moved by SQUARE_SHIFT into an empty 40 x 40 field."""
    return dataclasses.replace(open_field(200), path=fm.square_path() + SQUARE_SHIFT, name="square")


def model_rows(path, e, cpe, n_rivals):
    """The model's rows from the handle's read-backs."""
    prog, rs = e.progress(), e.race_steps()
    return rm.rival_rows(path, e.pose(), prog[:, 3], prog[:, 4], rs[:, 1], cpe, n_rivals)


def situations(path, rng, square):
    """Envs where the row can go wrong -- lists of (x, y, qw, qz, vx, vy), the first cars of an env -- then random ones."""
    P = lambda i: path[i % 100]
    out = []
    if square:          # the hand-written envs of the CPU test (the cars that race), exact on this path
        for cars in rm.hand_scenes().values():
            out.append([(x + SQUARE_SHIFT[0], y + SQUARE_SHIFT[1], q[0], q[1], vx, vy) for x, y, q, vx, vy, _, fin, _ in cars if not fin])
    for i in (6, 31, 99, 50, 77):
        a = np.round(0.5 * (P(i) + P(i + 1)) * 64.0) / 64.0           # few bits: a +- 0.25 and the differences are exact
        e = P(i + 1) - P(i)
        n = np.array([-e[1], e[0]]) / np.hypot(*e)
        yaw = rng.uniform(-np.pi, np.pi)
        q = (np.cos(yaw / 2), np.sin(yaw / 2))
        out.append([(a[0], a[1], *q, 1.0, 0.5), (a[0] + 0.25, a[1], *q, 0.0, 0.0), (a[0] - 0.25, a[1], *q, 2.0, -1.0)])           # equal d2
        out.append([(a[0], a[1], *q, 1.0, 0.5), (a[0], a[1], 1.0, 0.0, -1.0, 0.0), (a[0], a[1] + 0.5, *q, 0.0, 0.0)])               # one spot
        out.append([(a[0], a[1], *q, 0.0, 0.0), (a[0] + 3.0 * n[0], a[1] + 3.0 * n[1], *q, 0.0, 3.0)])                              # an off-track mate
    return out


def random_car(path, rng):
    i, w = int(rng.integers(100)), rng.uniform()
    p = (1 - w) * path[i] + w * path[(i + 1) % 100] + rng.uniform(-0.9, 0.9, 2)
    yaw = rng.uniform(-np.pi, np.pi)
    return (p[0], p[1], np.cos(yaw / 2), np.sin(yaw / 2), *rng.uniform(-4.0, 4.0, 2))


def put(base, cars):
    pose = base.copy()
    for k, (x, y, qw, qz, vx, vy) in enumerate(cars):
        pose[k, 0], pose[k, 1], pose[k, 3], pose[k, 6] = x, y, qw, qz
        pose[k, 7:] = 0.0
        pose[k, 7], pose[k, 8] = vx, vy
    return pose


def set_poses(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    square = opt["track"] == "square"
    t = square_track() if square else load_track(opt["track"])
    path = np.asarray(t.path, dtype=np.float64)
    rng = np.random.default_rng(17)
    pool = situations(path, rng, square)
    seen = dict(rows=0, d2_ties=0, one_spot=0, off_mates=0, padded=0, g_ties=0, wrapped=0)
    for n_envs, cpe in SHAPES:
        n = n_envs * cpe
        with capi.Env(lib, t, n_envs=n_envs, cars_per_env=cpe, n_rays=8, spawn_mode=0) as e:
            base = e.pose()
            rounds = min(6, -(-len(pool) // n_envs))
            for r in range(rounds):
                cars = []
                for k in range(n_envs):
                    sit = pool[(r * n_envs + k) % len(pool)][:cpe]
                    cars += sit + [random_car(path, rng) for _ in range(cpe - len(sit))]
                e.set_pose(put(base, cars))
                e.eval_progress()
                pose, prog, rs = e.pose(), e.progress(), e.race_steps()
                for n_rivals in SLOTS:
                    want = rm.rival_rows(path, pose, prog[:, 3], prog[:, 4], rs[:, 1], cpe, n_rivals)
                    got = e.get_rivals(n_rivals)
                    np.testing.assert_array_equal(got, want, err_msg=f"{t.name}: {n_envs} envs of {cpe}, round {r}, n_rivals {n_rivals}")
                np.testing.assert_array_equal(e.pose(), pose)
                # what the round held
                g, s, _, off = rm.progress64(path, pose, prog[:, 3])
                xy, fin = pose[:, 0:2].reshape(n_envs, cpe, 2), prog[:, 4].reshape(n_envs, cpe) != 0
                d = xy[:, None, :, :] - xy[:, :, None, :]
                d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
                mate = ~np.eye(cpe, dtype=bool)[None] & ~fin[:, None, :] & ~fin[:, :, None]
                for a in range(cpe):
                    for b in range(cpe):
                        for c in range(b + 1, cpe):
                            seen["d2_ties"] += int((mate[:, a, b] & mate[:, a, c] & (d2[:, a, b] == d2[:, a, c])).sum())
                seen["one_spot"] += int((mate & (d2 == 0.0)).sum())
                seen["off_mates"] += int((mate & off.reshape(n_envs, 1, cpe)).sum())
                ge, se = g.reshape(n_envs, cpe), s.reshape(n_envs, cpe)
                seen["g_ties"] += int((mate & (ge[:, None, :] == ge[:, :, None])).sum())
                seen["wrapped"] += int((mate & (np.abs(se[:, None, :] - se[:, :, None]) >= 50.0)).sum())
                seen["padded"] += int((want[:, 4 + 8 * 6 + rm.PRESENT] == 0.0).sum())
                seen["rows"] += n
            # the external rows at the current state: with rivals off the fixed entries, with the setter's n_rivals the whole rows
            roster = ["agent" if k % 2 == 0 else "lobotomy" for k in range(cpe)]
            ext = [k for k in range(cpe) if k % 2 == 0]
            e.device_io_config(roster, 0, 1, True)
            for on, n_rivals in ((False, 0), (True, 7), (True, 0)):
                if on:
                    e.device_io_rivals(True, n_rivals)
                w = 4 + 8 * n_rivals
                buf = torch.full((n_envs, len(ext), w), -7.0, dtype=torch.float32, device=DEV)
                e.rivals_device(buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                want = rm.rival_rows(path, pose, prog[:, 3], prog[:, 4], rs[:, 1], cpe, n_rivals).reshape(n_envs, cpe, w)[:, ext]
                np.testing.assert_array_equal(buf.cpu().numpy(), want, err_msg=f"ftgp_rivals_device, {n_envs} envs of {cpe}, n_rivals {n_rivals}")
    print(f"{t.name}: {seen}")
    assert seen["d2_ties"] > 0 and seen["one_spot"] > 0 and seen["off_mates"] > 0 and seen["padded"] > 0
    print("set poses ok")


def finished(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from tests.crowded_model import FINISHERS, finish_by_teleport
    lib, t, cpe = capi.load(), load_track("track"), 8
    path = np.asarray(t.path, dtype=np.float64)
    with capi.Env(lib, t, n_envs=2, cars_per_env=cpe, n_rays=8, spawn_mode=0, lap_target=1) as e:
        e.step(1)
        finish_by_teleport((e,), t, cpe)
        prog, rs = e.progress(), e.race_steps()
        done = np.zeros(2 * cpe, dtype=bool)
        for env, slot in FINISHERS:
            done[env * cpe + slot] = True
        np.testing.assert_array_equal(prog[:, 4] != 0, done, err_msg="who has finished")
        winners = e.winners().reshape(-1)
        assert (winners[done] > 0).all() and (winners[~done] == 0).all()
        for n_rivals in SLOTS:
            got = e.get_rivals(n_rivals)
            np.testing.assert_array_equal(got, model_rows(path, e, cpe, n_rivals), err_msg=f"n_rivals {n_rivals}")
        np.testing.assert_array_equal(got[done, rm.PLACE], winners[done].astype(np.float32), err_msg="a finished car's place")
        _, _, place, mates = rm.rival_rows64(path, e.pose(), prog[:, 3], prog[:, 4], rs[:, 1], cpe, 7)
        racing = (~done).reshape(2, cpe).sum(axis=1).repeat(cpe)
        present = (got[:, 4:].reshape(-1, 7, 8)[:, :, rm.PRESENT] == 1.0).sum(axis=1)
        np.testing.assert_array_equal(present, np.where(done, 0, racing - 1), err_msg="the mates are the cars that race")
        np.testing.assert_array_equal(got[:, rm.N_RACING], racing.astype(np.float32))
        for a in range(2 * cpe):
            listed = [int(b) for b in mates[a] if b >= 0]
            assert not any(done[a // cpe * cpe + b] for b in listed), f"car {a} lists a finished mate"
        assert (place[~done] > done.reshape(2, cpe).sum(axis=1).repeat(cpe)[~done]).all()      # every finisher is ahead of every racing car
    print("finished ok")


def actions(n_envs, n_agents, calls, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((calls, n_envs, n_agents, 2), generator=g)
    a[..., 0] = 0.5 + 3.5 * a[..., 0]                    # speed: the agents of an env drive at different speeds, places change
    a[..., 1] = 0.8 * (a[..., 1] - 0.5)                  # steering angle
    return a.to(DEV)


def closed_loop(opt):
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    path = np.asarray(load_track("track").path, dtype=np.float64)
    cpe, ext, n_envs, R, w = 4, [0, 2], 37, 3, 0.5
    pen = dict(off_track_penalty=0.25, wall_contact_penalty=0.125, car_contact_penalty=0.375)
    kw = dict(n_envs=n_envs, n_rays=64, cars_per_env=cpe, roster=["agent", "fast", "agent", "nidc"], scan_pool=2, scan_max_range=10.0, state=True,
              contacts=True, lookahead=4, lookahead_stride=3, dense_progress=True, random_start=True, start_lateral=0.8, max_episode_steps=40,
              action_repeat=2, **pen)
    X = DeviceVecEnv("track", n_rivals=R, place_reward=w, **kw)
    Z = DeviceVecEnv("track", n_rivals=R, **kw)                                 # without the place reward: the reward of T
    T = DeviceVecEnv("track", **kw)                                             # without rivals: nothing else may change
    N = DeviceVecEnv("track", n_rivals=R, place_reward=w, auto_reset=False, **kw)      # without auto-reset: the records before a reset
    assert X.rivals and X.rival.shape == (n_envs, 2, 4 + 8 * R) and Z.rivals and not T.rivals and T.rival is None
    calls = int(opt.get("calls", 120))
    act = actions(n_envs, 2, calls, 5)

    def agents(a):
        return a.reshape(n_envs, cpe, *a.shape[1:])[:, ext]

    def records(v):
        prog, rs = v.env.progress(), v.env.race_steps()
        return v.env.pose(), prog, rs[:, 1]

    def rows_at(rec, n_rivals=R):
        pose, prog, fs = rec
        return rm.rival_rows64(path, pose, prog[:, 3], prog[:, 4], fs, cpe, n_rivals)

    twins = (X, Z, T, N)
    for v in twins:
        v.reset()
    torch.cuda.synchronize()
    rec = records(X)
    np.testing.assert_array_equal(X.rival.cpu().numpy(), agents(rows_at(rec)[0].astype(np.float32)), err_msg="rival after reset()")
    seen = dict(resets=0, place_changes=0, gained=0, lost=0, mates=0, finished=0)
    for call in range(calls):
        pose0, prog0, _ = rec
        fin0 = prog0[:, 4] != 0
        _, s0, off0, _, _ = fm.frame_rows64(path, pose0)
        p0 = rows_at(rec)[2]
        np.testing.assert_array_equal(N.env.pose(), pose0, err_msg=f"the twins part before call {call}")
        for v in twins:
            v.step(act[call])
        torch.cuda.synchronize()
        before = records(N)                                             # after the steps, before any reset
        ended = (X.terminated | X.truncated).cpu().numpy()
        np.testing.assert_array_equal(ended, (N.terminated | N.truncated).cpu().numpy())
        rec = records(X)
        rows1, _, p1, _ = rows_at(before)
        rows1 = agents(rows1.astype(np.float32))
        rival, final = X.rival.cpu().numpy(), X.final_rival.cpu().numpy()
        np.testing.assert_array_equal(rival[~ended], rows1[~ended], err_msg=f"rival, call {call}")
        np.testing.assert_array_equal(final[ended], rows1[ended], err_msg=f"final_rival, call {call}")
        np.testing.assert_array_equal(N.rival.cpu().numpy(), rows1, err_msg=f"rival of the twin without auto-reset, call {call}")
        np.testing.assert_array_equal(rival, agents(rows_at(rec)[0].astype(np.float32)), err_msg=f"rival at the records read back (spawn state of a reset env), call {call}")
        # the reward: the dense base, the three penalties in their order, then the place term
        _, s1, off1, _, _ = fm.frame_rows64(path, before[0])
        contact = N.contact.cpu().numpy()                              # rows at the pose after the steps
        base = agents(fm.dense_reward(s0, off0, s1, off1, fin0))
        want = fm.penalised(base, agents(before[1][:, 5]) != 0, pen["off_track_penalty"], contact[:, :, 2] > 0, pen["wall_contact_penalty"],
                            contact[:, :, 3] > 0, pen["car_contact_penalty"])
        np.testing.assert_array_equal(T.reward.cpu().numpy(), want, err_msg=f"reward without rivals, call {call}")
        want = rm.place_reward(want, w, agents(p0), agents(p1), agents(fin0))
        np.testing.assert_array_equal(X.reward.cpu().numpy(), want, err_msg=f"reward, call {call}")
        np.testing.assert_array_equal(Z.reward.cpu().numpy(), T.reward.cpu().numpy(), err_msg=f"reward with place_reward 0, call {call}")
        for name in ("obs", "state", "final_state", "contact", "final_contact", "frame", "final_frame", "terminated", "truncated", "final_obs"):
            for v in (X, Z):
                np.testing.assert_array_equal(getattr(v, name).cpu().numpy(), getattr(T, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        np.testing.assert_array_equal(Z.rival.cpu().numpy(), rival, err_msg=f"rival with place_reward 0, call {call}")
        np.testing.assert_array_equal(Z.final_rival.cpu().numpy(), final, err_msg=f"final_rival with place_reward 0, call {call}")
        dp = agents(np.where(fin0, 0, p0 - p1))
        seen["resets"] += int(ended.sum()); seen["place_changes"] += int((dp != 0).sum()); seen["gained"] += int((dp > 0).sum()); seen["lost"] += int((dp < 0).sum())
        seen["mates"] += int((rows1[:, :, 4 + rm.PRESENT] == 1.0).sum()); seen["finished"] += int(agents(before[1][:, 4] != 0).sum())
        if ended.any():
            N.env.reset(ended)
    print(f"closed loop: {calls} calls, {seen}")
    assert seen["resets"] >= 1 and seen["place_changes"] >= 1 and seen["mates"] > 0
    for v in twins:
        v.close()
    print("closed loop ok")


def multi_track(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    n_envs, cpe, R = 7, 3, 2
    X = DeviceVecEnv(["small-circle", "track"], n_envs=n_envs, n_rays=16, cars_per_env=cpe, n_rivals=R, max_episode_steps=0)
    paths = [np.asarray(t.path, dtype=np.float64) for t in X.tracks]
    assert X.envs_per_track == (4, 3) and not np.array_equal(paths[0], paths[1])
    X.reset()
    act = actions(n_envs, cpe, 12, 9)
    for call in range(13):
        torch.cuda.synchronize()
        pose, prog, fs = X.env.pose(), X.env.progress(), X.env.race_steps()[:, 1]
        want, _, _ = rm.rival_rows_blocks(paths, X.envs_per_track, cpe, pose, prog[:, 3], prog[:, 4], fs, R)
        np.testing.assert_array_equal(X.rival.cpu().numpy().reshape(-1, 4 + 8 * R), want, err_msg=f"rival before call {call}")
        np.testing.assert_array_equal(X.env.get_rivals(R), want, err_msg=f"ftgp_get_rivals before call {call}")
        wrong, _, _ = rm.rival_rows_blocks(paths[::-1], X.envs_per_track, cpe, pose, prog[:, 3], prog[:, 4], fs, R)
        assert (wrong != want).any()                                    # the other track's path gives other rows
        if call < 12:
            X.step(act[call])
    X.close()
    print("multi track ok")


def off(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    n_envs, cpe = 16, 2
    kw = dict(n_envs=n_envs, n_rays=120, cars_per_env=cpe, max_episode_steps=30, lap_target=1, spawn_mode=1, seed=7)
    Y = DeviceVecEnv("small-circle", **kw)                                # built before the setter was ever called
    X = DeviceVecEnv("small-circle", rivals=False, **kw)
    assert not X.rivals and X.rival is None
    E = X.env
    refused(ARG, "n_rivals 8 through the binding", E.device_io_rivals, True, 8)
    E.device_io_rivals(True, 3, 0.5)
    E.device_io_rivals(False)
    fn, old = E.lib.fn("step_device_rivals"), Y.env.lib.fn("step_device_frame")
    calls = int(opt.get("calls", 80))
    act = actions(n_envs, cpe, calls, 3)
    X.reset(); Y.reset()
    ends = 0
    for call in range(calls):
        for v in (X, Y):
            v._check_actions(act[call])
            v._io.action, v._io.stream = act[call].data_ptr(), torch.cuda.current_stream(v.device).cuda_stream
        E.lib.check(fn(E.h, X._io_ref, None, None, None, None))
        Y.env.lib.check(old(Y.env.h, Y._io_ref, None, None, None))
        torch.cuda.synchronize()
        for name in ("obs", "reward", "terminated", "truncated", "final_obs"):
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(Y, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        ends += int((X.terminated | X.truncated).sum())
    np.testing.assert_array_equal(E.pose(), Y.env.pose())
    np.testing.assert_array_equal(E.progress(), Y.env.progress())
    assert ends > 0

    # ---- what must be refused
    lib, track = capi.load(), load_track("small-circle")
    path = np.asarray(track.path, dtype=np.float64)
    with capi.Env(lib, track, n_envs=4, cars_per_env=2, n_rays=8) as e:
        refused(STATE, "rivals before device_io_config", e.device_io_rivals, True)
        refused(STATE, "rivals off before device_io_config", e.device_io_rivals, False)
        buf = torch.zeros(8 * 4, device=DEV)
        refused(STATE, "rivals_device before device_io_config", e.rivals_device, buf.data_ptr())
        assert e.get_rivals(3).shape == (8, 28)                         # the read-back works on any handle
        out = np.zeros((8, 60), dtype=np.float32)
        for n_rivals in (-1, 8):
            assert lib.fn("get_rivals")(e.h, n_rivals, out.ctypes.data_as(ctypes.c_void_p)) == ARG, n_rivals
    ptrs = [act[0].data_ptr(), X.obs.data_ptr(), X.reward.data_ptr(), X.terminated.data_ptr(), X.truncated.data_ptr()]
    rows = torch.full((n_envs, cpe, 4 + 8 * 7), -7.0, dtype=torch.float32, device=DEV)
    final = torch.full_like(rows, -7.0)

    def snapshot():
        torch.cuda.synchronize()
        return (E.steps(), E.pose(), E.progress(), X.obs.cpu().numpy(), X.reward.cpu().numpy(), rows.cpu().numpy(), final.cpu().numpy())
    before = snapshot()
    refused(STATE, "rival buffers while rivals are off", E.step_device_rivals, *ptrs, rival=rows.data_ptr())
    refused(STATE, "a final_rival buffer while rivals are off", E.step_device_rivals, *ptrs, final_rival=final.data_ptr())
    E.device_io_rivals(True, 2, 0.0)
    for what, (n_rivals, reserved, weight, reserved_f) in (("n_rivals -1", (-1, 0, 0.0, 0.0)), ("n_rivals 8", (8, 0, 0.0, 0.0)),
                                                           ("a negative weight", (2, 0, -0.5, 0.0)), ("a NaN weight", (2, 0, float("nan"), 0.0)),
                                                           ("an infinite weight", (2, 0, float("inf"), 0.0)), ("reserved 1", (2, 1, 0.0, 0.0)),
                                                           ("reserved_f 1", (2, 0, 0.0, 1.0))):
        r = capi.FtgpDeviceRivals(n_rivals, reserved, weight, reserved_f)
        assert E.lib.fn("device_io_rivals")(E.h, ctypes.byref(r)) == ARG, what
    host = np.zeros((n_envs, cpe, 20), dtype=np.float32)
    refused(ARG, "a host pointer for rival", E.step_device_rivals, *ptrs, rival=host.ctypes.data)
    refused(ARG, "a host pointer for final_rival", E.step_device_rivals, *ptrs, rival=rows.data_ptr(), final_rival=host.ctypes.data)
    refused(ARG, "a host pointer for ftgp_rivals_device", E.rivals_device, host.ctypes.data)
    for x, y in zip(before, snapshot()):          # nothing was enqueued by a refused call, and a refused setter left {2, 0, 0, 0} alone
        np.testing.assert_array_equal(x, y)

    def step_and_check(n_rivals, what):
        E.step_device_rivals(*ptrs, rival=rows.data_ptr(), final_rival=final.data_ptr())
        torch.cuda.synchronize()
        w = 4 + 8 * n_rivals
        got = rows.cpu().numpy().reshape(-1)[:n_envs * cpe * w].reshape(n_envs * cpe, w)
        np.testing.assert_array_equal(got, model_rows(path, E, cpe, n_rivals), err_msg=what)
    step_and_check(2, "the setter's n_rivals")
    E.device_io_signals(1, 0.0); E.device_io_contacts(True); E.device_io_contacts(False); E.device_io_frame(True, 2, 5); E.device_io_frame(False)
    step_and_check(2, "after the signals, contacts and frame setters")
    E.lib.check(E.lib.fn("device_io_rivals")(E.h, ctypes.byref(capi.FtgpDeviceRivals(0, 0, 0.0, 0.0))))
    step_and_check(0, "{0, 0, 0, 0} still turns the fixed entries on")
    E.step_device_rivals(*ptrs)                                         # rows work without buffers
    E.device_io_config(None, 30, 1, True)                               # ... and a later device_io_config turns rivals off
    refused(STATE, "rival buffers after a later device_io_config", E.step_device_rivals, *ptrs, rival=rows.data_ptr())
    E.step_device_rivals(*ptrs)
    torch.cuda.synchronize()
    X.close(); Y.close()
    print(f"off ok: {ends} episode ends")


SCENARIOS = {"set_poses": set_poses, "finished": finished, "closed_loop": closed_loop, "multi_track": multi_track, "off": off}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
