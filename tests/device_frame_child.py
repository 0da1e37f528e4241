"""Child process of tests/test_device_frame.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/device_frame_child.py <scenario> [json options]

`set_poses`: poses put with set_pose; ftgp_get_frames and ftgp_frame_device against the numpy model of the header
(tests/frame_model.py), bit for bit.
`closed_loop`: a DeviceVecEnv with every signal on against the model at the poses read back at every call, with a twin without the
frame (state, contact) and a twin without auto-reset (the poses before a reset).
`multi_track`, `off`, `integer`: rows follow each env's own path; the frame off is the old call, and what must be refused; the frame
without dense_progress keeps the integer reward.
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
from tests.device_twin import refused  # noqa: E402
from tests.helpers import open_field  # noqa: E402

DEV = "cuda:0"
STATE, ARG = -4, -1          # FTGP_ERR_STATE, FTGP_ERR_ARG
COUNTS = (1, 15, 16, 17, 37)
AHEAD, STRIDES = (0, 1, 16), (1, 7, 50)


def put(pose, rows):
    """(x, y, yaw) per car into rows of ftgp_get_pose, at rest."""
    pose = pose.copy()
    for k, (x, y, yaw) in enumerate(rows):
        pose[k, 0], pose[k, 1], pose[k, 3], pose[k, 6] = x, y, np.cos(yaw / 2), np.sin(yaw / 2)
        pose[k, 7:] = 0.0
    return pose


def square_track():
    """`skew_path` of tests/frame_model.py in an empty 40 x 40 field: the hand-written square with point 11 on point 10, and with
    point 99 moved so that outside the corner at point 0 rounding takes segment 99 -> 0 with t = 1 and s wraps."""
    return dataclasses.replace(open_field(200), path=fm.skew_path(), name="square")


def pose_pool(path, rng, square):
    """Poses where the row can go wrong, then random ones along the path."""
    P = lambda i: path[i % 100]
    mid = lambda i: 0.5 * (P(i) + P(i + 1))
    pool = []
    for i in (6, 0, 99, 98, 24, 25, 49, 50, 74, 75):
        n = np.array([-(P(i + 1) - P(i))[1], (P(i + 1) - P(i))[0]])
        for lat in (0.0, 0.25, -0.25):
            pool.append((*(mid(i) + lat * n), 0.0))              # equidistant from two points: the first minimum
            pool.append((*(P(i) + lat * n), np.pi))              # on a point, on its normal: the A / B tie
    for i in (0, 25, 50, 75, 99):                                # around the corners (of the square), inside and outside
        for dx, dy in ((0.5, 0.5), (-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5), (0.125, -0.125)):
            pool.append((P(i)[0] + dx, P(i)[1] + dy, 0.7))
    if square:
        pool += [(*fm.SKEW_WRAP_POSE, 0.3), (P(0)[0] - 0.125, P(0)[1] - 0.5, -2.5)]                 # a = 99 with t = 1 by rounding: s wraps to 0
        pool += [(P(10)[0], P(10)[1] + 0.25, 0.0), (P(10)[0] + 0.125, P(10)[1] - 0.25, 2.0), (P(11)[0], P(11)[1], -1.0)]     # the duplicated point
    for i in (3, 40, 77):                                        # off the track
        pool += [(P(i)[0] + 3.0, P(i)[1] - 2.0, 1.0), (P(i)[0] - 1.0, P(i)[1] + 0.25, -2.0)]
    for _ in range(80):
        i, w = int(rng.integers(100)), rng.uniform()
        q = (1 - w) * P(i) + w * P(i + 1) + rng.uniform(-0.9, 0.9, 2)
        pool.append((q[0], q[1], rng.uniform(-np.pi, np.pi)))
    return pool


def set_poses(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    lib = capi.load()
    square = opt["track"] == "square"
    t = square_track() if square else load_track(opt["track"])
    path = np.asarray(t.path, dtype=np.float64)
    rng = np.random.default_rng(11)
    pool = pose_pool(path, rng, square)
    seen = dict(rows=0, off=0, took_a=0, c0=0, c99=0, flat=0, wrapped=0)
    for n in COUNTS:
        with capi.Env(lib, t, n_envs=n, cars_per_env=1, n_rays=8) as e:
            base = e.pose()
            starts = list(range(0, len(pool), n))[:6] if n > 1 else list(range(0, len(pool), 3))
            for r, first in enumerate(starts):
                rows = (pool[first:first + n] + pool)[:n]
                e.set_pose(put(base, rows))
                pose = e.pose()
                for n_ahead in AHEAD:
                    for stride in STRIDES:
                        want = fm.frame_rows(path, pose, n_ahead, stride)
                        got = e.get_frames(n_ahead, stride)
                        np.testing.assert_array_equal(got, want, err_msg=f"{t.name}: {n} cars, round {r}, n_ahead {n_ahead}, stride {stride}")
                _, s, off, a, c = fm.frame_rows64(path, pose)
                seen["wrapped"] += int(((a == 99) & (s == 0.0)).sum())
                seen["rows"] += n; seen["off"] += int(off.sum()); seen["took_a"] += int((a != c).sum())
                seen["c0"] += int((c == 0).sum()); seen["c99"] += int((c == 99).sum())
                seen["flat"] += int(((c == 10) | (c == 11)).sum()) if square else 0
                np.testing.assert_array_equal(e.pose(), pose)
            # the external rows at the current state, with the setter's n_ahead and stride; with the frame off, the fixed entries
            e.device_io_config(None, 0, 1, True)
            for on, n_ahead, stride in ((False, 0, 1), (True, 16, 7), (True, 0, 1)):
                if on:
                    e.device_io_frame(True, n_ahead, stride)
                buf = torch.full((n, 1, fm.FRAME_FIXED + 2 * n_ahead), -7.0, dtype=torch.float32, device=DEV)
                e.frame_device(buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(buf.cpu().numpy()[:, 0], fm.frame_rows(path, pose, n_ahead, stride), err_msg=f"ftgp_frame_device, {n} cars")
    print(f"{t.name}: {seen}")
    assert seen["off"] > 0 and seen["took_a"] > 0 and seen["c0"] > 0 and seen["c99"] > 0 and ((seen["flat"] > 0 and seen["wrapped"] > 0) or not square)
    print("set poses ok")


def actions(n_envs, n_agents, calls, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((calls, n_envs, n_agents, 2), generator=g)
    a[..., 0] = 1.0 + 3.0 * a[..., 0]                    # speed
    a[..., 1] = 0.8 * (a[..., 1] - 0.5)                  # steering angle
    return a.to(DEV)


def closed_loop(opt):
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    track = load_track("small-circle")
    path = np.asarray(track.path, dtype=np.float64)
    cpe, ext, n_envs, L, stride = 3, [0, 2], 5, 4, 3
    kw = dict(n_envs=n_envs, n_rays=64, cars_per_env=cpe, roster=["agent", "nidc", "agent"], state=True, contacts=True, random_start=True,
              start_lateral=0.8, max_episode_steps=40, action_repeat=2)
    X = DeviceVecEnv("small-circle", lookahead=L, lookahead_stride=stride, dense_progress=True, **kw)
    T = DeviceVecEnv("small-circle", **kw)                              # without the frame: state and contact must not change
    N = DeviceVecEnv("small-circle", auto_reset=False, **kw)            # without auto-reset: the poses before a reset
    assert X.track_frame and X.frame.shape == (n_envs, 2, 4 + 2 * L) and not T.track_frame and T.frame is None
    calls = int(opt.get("calls", 120))
    act = actions(n_envs, 2, calls, 5)

    def agents(a):
        return a.reshape(n_envs, cpe, *a.shape[1:])[:, ext]

    for v in (X, T, N):
        v.reset()
    torch.cuda.synchronize()
    pose = X.env.pose()
    np.testing.assert_array_equal(X.frame.cpu().numpy(), agents(fm.frame_rows(path, pose, L, stride)), err_msg="frame after reset()")
    seen = dict(resets=0, moved=0, frozen=0, backwards=0, across_the_line=0)
    for call in range(calls):
        fin0 = X.env.progress()[:, 4] != 0
        _, s0, off0, _, _ = fm.frame_rows64(path, pose)
        np.testing.assert_array_equal(N.env.pose(), pose, err_msg=f"the twins part before call {call}")
        for v in (X, T, N):
            v.step(act[call])
        torch.cuda.synchronize()
        before = N.env.pose()                                           # after the steps, before any reset
        ended = (X.terminated | X.truncated).cpu().numpy()
        np.testing.assert_array_equal(ended, (N.terminated | N.truncated).cpu().numpy())
        pose = X.env.pose()
        rows, s1, off1, _, _ = fm.frame_rows64(path, before, L, stride)
        rows = agents(rows.astype(np.float32))
        frame, final = X.frame.cpu().numpy(), X.final_frame.cpu().numpy()
        np.testing.assert_array_equal(frame[~ended], rows[~ended], err_msg=f"frame, call {call}")
        np.testing.assert_array_equal(agents(pose)[~ended], agents(before)[~ended])
        np.testing.assert_array_equal(final[ended], rows[ended], err_msg=f"final_frame, call {call}")
        np.testing.assert_array_equal(frame[ended], agents(fm.frame_rows(path, pose, L, stride))[ended], err_msg=f"frame at the spawn pose, call {call}")
        want = agents(fm.penalised(fm.dense_reward(s0, off0, s1, off1, fin0), np.zeros(len(s0))))
        np.testing.assert_array_equal(X.reward.cpu().numpy(), want, err_msg=f"reward, call {call}")
        for name in ("obs", "state", "final_state", "contact", "final_contact", "terminated", "truncated", "final_obs"):
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(T, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        seen["resets"] += int(ended.sum()); seen["moved"] += int((want != 0).sum()); seen["backwards"] += int((want < 0).sum())
        seen["frozen"] += int(agents(off0 | off1 | fin0).sum()); seen["across_the_line"] += int(agents(np.abs(s1 - s0) >= 50.0).sum())
        if ended.any():
            N.env.reset(ended)
    print(f"closed loop: {calls} calls, {seen}")
    assert seen["resets"] >= n_envs and seen["moved"] > calls
    for v in (X, T, N):
        v.close()
    print("closed loop ok")


def multi_track(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    n_envs, cpe, L, stride = 7, 8, 5, 3
    X = DeviceVecEnv(["small-circle", "circle"], n_envs=n_envs, n_rays=16, cars_per_env=cpe, lookahead=L, lookahead_stride=stride,
                     max_episode_steps=0)
    paths = [np.asarray(t.path, dtype=np.float64) for t in X.tracks]
    assert X.envs_per_track == (4, 3) and not np.array_equal(paths[0], paths[1])
    X.reset()
    act = actions(n_envs, cpe, 12, 9)
    for call in range(13):
        torch.cuda.synchronize()
        pose = X.env.pose()
        want, _, _ = fm.frame_blocks(paths, X.envs_per_track, cpe, pose, L, stride)
        np.testing.assert_array_equal(X.frame.cpu().numpy().reshape(-1, 4 + 2 * L), want, err_msg=f"frame before call {call}")
        np.testing.assert_array_equal(X.env.get_frames(L, stride), want, err_msg=f"ftgp_get_frames before call {call}")
        wrong, _, _ = fm.frame_blocks(paths[::-1], X.envs_per_track, cpe, pose, L, stride)
        assert (wrong != want).any()                                    # the other track's path gives other rows
        if call < 12:
            X.step(act[call])
    X.close()
    print("multi track ok")


def _pair(kw_x, kw_y, **kw):
    from ft_grandprix_amd.vec import DeviceVecEnv
    Y = DeviceVecEnv("small-circle", **kw, **kw_y)
    X = DeviceVecEnv("small-circle", **kw, **kw_x)
    return X, Y


def off(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    kw = dict(n_envs=16, n_rays=120, max_episode_steps=30, lap_target=1, spawn_mode=1, seed=7)
    X, Y = _pair(dict(track_frame=False), {}, **kw)                     # Y: built before the setter was ever called
    assert not X.track_frame and X.frame is None
    E = X.env
    E.device_io_frame(True, 8, 3, True)
    E.device_io_frame(False)
    fn = E.lib.fn("step_device_frame")
    calls = int(opt.get("calls", 80))
    act = actions(16, 1, calls, 3)
    X.reset(); Y.reset()
    ends = 0
    for call in range(calls):
        X._check_actions(act[call])
        X._io.action, X._io.stream = act[call].data_ptr(), torch.cuda.current_stream(X.device).cuda_stream
        E.lib.check(fn(E.h, X._io_ref, None, None, None))
        Y.step(act[call])
        torch.cuda.synchronize()
        for name in ("obs", "reward", "terminated", "truncated", "final_obs"):
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(Y, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        ends += int((X.terminated | X.truncated).sum())
    np.testing.assert_array_equal(E.pose(), Y.env.pose())
    assert ends > 0

    # ---- what must be refused
    lib, track = capi.load(), load_track("small-circle")
    with capi.Env(lib, track, n_envs=8, n_rays=8) as e:
        refused(STATE, "the frame before device_io_config", e.device_io_frame, True)
        refused(STATE, "the frame off before device_io_config", e.device_io_frame, False)
        buf = torch.zeros(8 * 4, device=DEV)
        refused(STATE, "frame_device before device_io_config", e.frame_device, buf.data_ptr())
        assert e.get_frames(3, 2).shape == (8, 10)                      # the read-back works on any handle
        out = np.zeros((8, 36), dtype=np.float32)
        for n_ahead, stride in ((-1, 1), (17, 1), (0, 0), (0, 51), (4, -2)):
            assert lib.fn("get_frames")(e.h, n_ahead, stride, out.ctypes.data_as(ctypes.c_void_p)) == ARG, (n_ahead, stride)
    ptrs = [act[0].data_ptr(), X.obs.data_ptr(), X.reward.data_ptr(), X.terminated.data_ptr(), X.truncated.data_ptr()]
    rows = torch.full((16, 1, 4 + 2 * 16), -7.0, dtype=torch.float32, device=DEV)
    final = torch.full_like(rows, -7.0)

    def snapshot():
        torch.cuda.synchronize()
        return (E.steps(), E.pose(), E.progress(), X.obs.cpu().numpy(), X.reward.cpu().numpy(), rows.cpu().numpy(), final.cpu().numpy())
    before = snapshot()
    refused(STATE, "frame buffers while the frame is off", E.step_device_frame, *ptrs, frame=rows.data_ptr())
    refused(STATE, "a final_frame buffer while the frame is off", E.step_device_frame, *ptrs, final_frame=final.data_ptr())
    E.device_io_frame(True, 2, 5, False)
    for what, (n_ahead, stride, reserved) in (("n_ahead -1", (-1, 1, 0)), ("n_ahead 17", (17, 1, 0)), ("stride 0", (2, 0, 0)),
                                              ("stride 51", (2, 51, 0)), ("reserved 1", (2, 1, 1))):
        f = capi.FtgpDeviceFrame(n_ahead, stride, 1, reserved)
        assert E.lib.fn("device_io_frame")(E.h, ctypes.byref(f)) == ARG, what
    host = np.zeros((16, 1, 8), dtype=np.float32)
    refused(ARG, "a host pointer for frame", E.step_device_frame, *ptrs, frame=host.ctypes.data)
    refused(ARG, "a host pointer for final_frame", E.step_device_frame, *ptrs, frame=rows.data_ptr(), final_frame=host.ctypes.data)
    refused(ARG, "a host pointer for ftgp_frame_device", E.frame_device, host.ctypes.data)
    for x, y in zip(before, snapshot()):          # nothing was enqueued by a refused call, and a refused setter left {2, 5, 0} alone
        np.testing.assert_array_equal(x, y)
    path = np.asarray(track.path, dtype=np.float64)

    def step_and_check(n_ahead, stride, what):
        E.step_device_frame(*ptrs, frame=rows.data_ptr(), final_frame=final.data_ptr())
        torch.cuda.synchronize()
        ended = (X.terminated | X.truncated).cpu().numpy()
        w = 4 + 2 * n_ahead
        got = rows.cpu().numpy().reshape(-1)[:16 * w].reshape(16, w)
        np.testing.assert_array_equal(got, fm.frame_rows(path, E.pose(), n_ahead, stride), err_msg=what)
        return ended
    step_and_check(2, 5, "the setter's n_ahead and stride")
    E.device_io_signals(1, 0.0); E.device_io_contacts(True); E.device_io_contacts(False)       # they leave the frame alone
    step_and_check(2, 5, "after the signals and contacts setters")
    E.lib.check(E.lib.fn("device_io_frame")(E.h, ctypes.byref(capi.FtgpDeviceFrame(0, 1, 0, 0))))
    step_and_check(0, 1, "{0, 1, 0, 0} still turns the fixed entries on")
    E.step_device_frame(*ptrs)                                          # dense_progress and rows work without buffers
    E.device_io_config(None, 30, 1, True)                               # ... and a later device_io_config turns the frame off
    refused(STATE, "frame buffers after a later device_io_config", E.step_device_frame, *ptrs, frame=rows.data_ptr())
    E.step_device_frame(*ptrs)
    torch.cuda.synchronize()
    X.close(); Y.close()
    print(f"off ok: {ends} episode ends")


def integer(opt):
    from ft_grandprix_amd.track import load_track
    kw = dict(n_envs=16, n_rays=120, max_episode_steps=200, action_repeat=10, lap_target=1, spawn_mode=1, seed=7, off_track_penalty=0.5)
    X, Y = _pair(dict(track_frame=True, lookahead=2, lookahead_stride=50), {}, **kw)
    assert X.track_frame and not X.dense_progress and X.frame.shape == (16, 1, 8)
    path = np.asarray(load_track("small-circle").path, dtype=np.float64)
    calls = int(opt.get("calls", 80))
    act = actions(16, 1, calls, 4)
    X.reset(); Y.reset()
    ends = moved = 0
    for call in range(calls):
        X.step(act[call]); Y.step(act[call])
        torch.cuda.synchronize()
        for name in ("obs", "reward", "terminated", "truncated", "final_obs"):
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(Y, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        np.testing.assert_array_equal(X.frame.cpu().numpy()[:, 0], fm.frame_rows(path, X.env.pose(), 2, 50), err_msg=f"frame, call {call}")
        r = X.reward.cpu().numpy()
        ends += int((X.terminated | X.truncated).sum()); moved += int((r != 0).sum())
    assert ends > 0 and moved > 0
    X.close(); Y.close()
    print(f"integer ok: {ends} episode ends, {moved} rewards other than zero")


def frozen(opt):
    """Dense progress with cars put off the track, and cars put just before the line: the reward is frozen for the ones, wraps for the
    others, and the off-track penalty comes off it."""
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    path = np.asarray(load_track("small-circle").path, dtype=np.float64)
    n = 12
    X = DeviceVecEnv("small-circle", n_envs=n, n_rays=16, dense_progress=True, off_track_penalty=0.5, action_repeat=5, max_episode_steps=0)
    X.reset()
    rows = []
    for k in range(n):
        i = (99 + k) % 100 if k < 6 else 7 * k + 20
        e = path[(i + 1) % 100] - path[i]
        u = e / np.hypot(*e)
        lat = (0.0, 1.5, -1.5, 0.9)[k % 4]                     # on the centre-line; off the track to either side; near its edge
        rows.append((*(path[i] + 0.7 * e + lat * np.array([-u[1], u[0]])), np.arctan2(e[1], e[0]) + (np.pi if k % 6 == 5 else 0.0)))
    X.env.set_pose(put(X.env.pose(), rows))
    X.env.eval_progress()
    act = actions(n, 1, 10, 2)
    seen = dict(frozen=0, across_the_line=0, backwards=0, moved=0)
    for call in range(10):
        pose0 = X.env.pose()
        fin0 = X.env.progress()[:, 4] != 0
        _, s0, off0, _, _ = fm.frame_rows64(path, pose0)
        X.step(act[call])
        torch.cuda.synchronize()
        _, s1, off1, _, _ = fm.frame_rows64(path, X.env.pose())
        base = fm.dense_reward(s0, off0, s1, off1, fin0)
        want = fm.penalised(base, X.env.progress()[:, 5] != 0, 0.5)
        np.testing.assert_array_equal(X.reward.cpu().numpy()[:, 0], want, err_msg=f"reward, call {call}")
        np.testing.assert_array_equal((X.terminated | X.truncated).cpu().numpy(), np.zeros(n, dtype=bool))
        seen["frozen"] += int((off0 | off1).sum()); seen["across_the_line"] += int((np.abs(s1 - s0) >= 50.0).sum())
        seen["backwards"] += int((base < 0).sum()); seen["moved"] += int((base != 0).sum())
    print(f"frozen: {seen}")
    assert seen["frozen"] > 0 and seen["across_the_line"] > 0 and seen["moved"] > 0
    X.close()
    print("frozen ok")


SCENARIOS = {"frozen": frozen, "set_poses": set_poses, "closed_loop": closed_loop, "multi_track": multi_track, "off": off, "integer": integer}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
