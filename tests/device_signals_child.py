"""Child process of tests/test_device_signals.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/device_signals_child.py <scenario> [json options]

`twin`: a DeviceVecEnv with signals (handle A) against a twin handle B on the host path, bit for bit at every call.  What A must
write is modelled in numpy (tests/signals_model.py) from B's host read-backs alone -- lidar(), pose(), ctrl(), progress(),
centre_dist2(), steps() -- so every count the scenario asserts (`need`) is a count of B's data.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import signals_model as sm  # noqa: E402


def _spawn_point(env, car):
    return (10 + 7 * env + 2 * car) % 98          # spawn_mode 1 (ftgp_reset_kernel)


def _same_pose(handles):
    pose = handles[0].pose()
    for h in handles[1:]:
        np.testing.assert_array_equal(h.pose(), pose)
    return pose


def _apply(handles, pose):
    for h in handles:
        h.set_pose(pose)
        h.eval_progress()


def teleport(handles, paths, envs, cars, cpe):
    """The given cars, on every handle alike, to the last centre-line point of their lap (through 40 % and 80 % of it, so that the
    progress rule counts no crossing), rolling along the line at 3 units/s: a short drive then finishes the lap."""
    pose = _same_pose(handles)
    for frac in (40, 80, 99):
        for e in envs:
            for c in cars:
                path = paths[e]
                q = (_spawn_point(e, c) + frac) % 100
                a = np.arctan2(path[(q + 1) % 100, 1] - path[q, 1], path[(q + 1) % 100, 0] - path[q, 0])
                row = pose[e * cpe + c]
                row[0], row[1], row[3], row[6] = path[q, 0], path[q, 1], np.cos(a / 2), np.sin(a / 2)
                row[7], row[8], row[12] = 3.0 * np.cos(a), 3.0 * np.sin(a), 0.0
        _apply(handles, pose)


def push_off(handles, paths, envs, cars, cpe, dist=1.5):
    """The given cars, on every handle alike, `dist` units off the centre-line, along the normal at the point nearest to them."""
    pose = _same_pose(handles)
    for e in envs:
        for c in cars:
            path, row = paths[e], pose[e * cpe + c]
            q = int(((path - row[0:2]) ** 2).sum(axis=1).argmin())
            t = path[(q + 1) % 100] - path[(q - 1) % 100]
            n = np.array([-t[1], t[0]]) / np.hypot(t[0], t[1])
            row[0], row[1] = path[q, 0] + dist * n[0], path[q, 1] + dist * n[1]
    _apply(handles, pose)


class HostTwin:
    """Handle B and what a device call must have written, from its host read-backs."""

    def __init__(self, B, roster, paths, pool, M, penalty, term_off, max_steps, repeat, auto_reset, dist2_of=None):
        self.B, self.roster, self.cpe = B, roster, len(roster)
        self.ext = [k for k, r in enumerate(roster) if r == "agent"]
        self.bundled = len(self.ext) < self.cpe
        self.car_paths = np.repeat(np.asarray(paths), self.cpe, axis=0)          # [n_cars, 100, 2]
        self.pool, self.M, self.penalty, self.term_off = pool, M, np.float32(penalty), term_off
        self.max_steps, self.repeat, self.auto_reset = max_steps, repeat, auto_reset
        self.dist2_of = dist2_of or (lambda b: b.centre_dist2())
        self.n = B.n_envs
        self.car_mask = np.zeros((self.n, self.cpe), dtype=np.uint8)
        self.car_mask[:, self.ext] = 1
        self.count = dict(off_term=0, fin_term=0, trunc=0, clipped=0, mixed=0, all_miss=0, penalised=0)
        if self.bundled:
            B.set_car_policies(["lobotomy" if r == "agent" else r for r in roster])

    def _ext(self, x):
        return x.reshape((self.n, self.cpe) + x.shape[1:])[:, self.ext]

    def state(self):
        B = self.B
        d2, pose, prog = self.dist2_of(B), B.pose(), B.progress()
        racing = prog[:, 4] == 0
        # the stored field is the model's value, to the bit: the same subtractions, squares, sum and comparisons (no fused operation)
        np.testing.assert_array_equal(d2[racing], sm.centre_dist2(pose, self.car_paths)[racing], err_msg="centre_dist2 against numpy")
        return self._ext(sm.state_rows(pose, B.ctrl(), prog, d2))

    def call(self, a):
        """One device call on B with actions a float64 [n_envs, n_ext, 2]; returns what A must hold."""
        B, n, cpe, ext = self.B, self.n, self.cpe, self.ext
        p0 = B.progress()
        for _ in range(self.repeat):
            fin = B.progress()[:, 4].reshape(n, cpe)
            ctrl = np.zeros((n, cpe, 2), dtype=np.float64)
            if self.bundled:
                ctrl = B.policy_eval("per_car", B.lidar()).reshape(n, cpe, 2)
            ctrl[:, ext] = np.where(fin[:, ext, None] != 0, 0.0, a)
            B.set_ctrl(ctrl, self.car_mask if self.bundled else None)
            B.step(1)
        p1 = B.progress()
        off = self._ext(p1[:, 5]) != 0
        reward = self._ext(p1[:, 3] - p0[:, 3]).astype(np.float32)
        reward = np.where(off, reward - self.penalty, reward).astype(np.float32)
        fin_all = (self._ext(p1[:, 4]) != 0).all(axis=1)
        term = fin_all | (bool(self.term_off) & off.any(axis=1))
        trunc = ~term & (self.max_steps > 0) & (B.steps() >= self.max_steps)
        lid = self._ext(B.lidar())
        obs = sm.pool_scan(lid, self.pool, self.M)
        state = self.state()
        ended = term | trunc
        out = dict(reward=reward, terminated=term, truncated=trunc, ended=ended, off=off, final_obs=None, final_state=None)
        if self.auto_reset and ended.any():
            out["final_obs"], out["final_state"] = obs[ended].copy(), state[ended].copy()
            B.reset(ended.astype(np.uint8))
            obs[ended] = 0.0
            state = self.state()                  # the spawn state of the envs just reset; the others' rows are what they were
        out["obs"], out["state"] = obs, state
        c = self.count
        c["off_term"] += int((term & ~fin_all).sum()); c["fin_term"] += int(fin_all.sum()); c["trunc"] += int(trunc.sum())
        mixed, all_miss, clipped = sm.beam_classes(lid, self.pool, self.M)
        c["mixed"] += mixed; c["all_miss"] += all_miss; c["clipped"] += clipped; c["penalised"] += int(off.sum())
        return out


def torch_driver(torch, obs, gen, dev):
    """The driver of tests/device_io_child.py on whatever the observation holds: steer towards the largest value of the front half,
    speed ~ U(0.5, 3); then noise, some of it past the ctrlrange."""
    n, k, nb = obs.shape
    front = obs[:, :, nb // 4: 3 * nb // 4]
    j = front.argmax(dim=2).float() / max(1, front.shape[2] - 1)
    steer = (j - 0.5) * 2.0
    speed = 0.5 + 2.5 * torch.rand((n, k), generator=gen, device=dev)
    act = torch.stack([speed, steer + 0.3 * torch.randn((n, k), generator=gen, device=dev)], dim=2)
    wild = torch.rand((n, k, 2), generator=gen, device=dev) < 0.05
    return torch.where(wild, 6.0 * torch.randn((n, k, 2), generator=gen, device=dev), act).contiguous()


def _tracks(opt):
    from ft_grandprix_amd.track import load_track
    names = opt.get("track", "small-circle")
    multi = isinstance(names, list)
    tracks = [sm.open_right_track() if t == "open-right" else load_track(t) for t in (names if multi else [names])]
    return (tracks if multi else tracks[0]), tracks


def _full_state(env):
    counts, times = env.lap_times()
    return dict(pose=env.pose(), progress=env.progress(), lap_counts=counts, lap_times=times, steps=env.steps(), lidar=env.lidar(),
                ctrl=env.ctrl(), dist2=env.centre_dist2(), race_steps=env.race_steps())


def _same_state(A, B):
    a, b = _full_state(A), _full_state(B)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"handle state at the end: {k}")


def twin(opt):
    import torch
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.vec import DeviceVecEnv

    n_envs, n_rays, cpe = opt.get("n_envs", 64), opt.get("n_rays", 120), opt.get("cars_per_env", 1)
    roster = opt.get("roster", ["agent"] * cpe)
    cpe = len(roster)
    pool, M, pen, term_off = opt.get("pool", 1), opt.get("M", 0.0), opt.get("penalty", 0.0), opt.get("terminate_off_track", False)
    R, max_steps, AR = opt.get("action_repeat", 1), opt.get("max_episode_steps", 200), opt.get("auto_reset", True)
    calls, side, epb = opt.get("calls", 300), opt.get("side_stream", False), opt.get("envs_per_track")
    kw = dict(lap_target=1, spawn_mode=1, seed=7)
    track, tracks = _tracks(opt)
    if epb is not None:
        kw["envs_per_track"] = epb
    dev = torch.device("cuda", 0)
    venv = DeviceVecEnv(track, n_envs=n_envs, n_rays=n_rays, cars_per_env=cpe, roster=roster, max_episode_steps=max_steps,
                        action_repeat=R, auto_reset=AR, device_id=0, scan_pool=pool, scan_max_range=M, state=True,
                        terminate_off_track=term_off, off_track_penalty=pen, **kw)
    assert venv.n_beams == n_rays // pool and tuple(venv.obs.shape) == (n_envs, roster.count("agent"), n_rays // pool)
    B = capi.Env(capi.load(), track, n_envs=n_envs, cars_per_env=cpe, n_rays=n_rays, **kw)
    A = venv.env
    paths = [np.asarray(tracks[t].path, dtype=np.float64) for t in A.track_of_env]
    host = HostTwin(B, roster, paths, pool, M, pen, term_off, max_steps, R, AR)
    ext, n_tracks = host.ext, len(tracks)
    gen = torch.Generator(device=dev)
    gen.manual_seed(opt.get("seed", 1))
    stream = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)

    def reset_both():
        with torch.cuda.stream(stream):
            o = venv.reset().clone()              # ftgp_state_device on `stream`; the clones follow it there without a host wait
            s = venv.state.clone()
        B.reset()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(s.cpu().numpy(), host.state(), err_msg="state after reset()")
        assert not o.cpu().numpy().any()
        return o

    obs = reset_both()
    off_term_of_track = np.zeros(n_tracks, dtype=np.int64)
    off_streak, term_streak, best_streak = np.zeros(n_envs, dtype=np.int64), np.zeros(n_envs, dtype=np.int64), [0, 0]
    for call in range(calls):
        if call % 60 == 5:                        # bring some cars to the end of their lap: finishes
            teleport([A, B], paths, [e for e in range(n_envs) if (e + call) % 5 == 0], ext, cpe)
        if call % 40 == 7:                        # and some off the track
            push_off([A, B], paths, [e for e in range(n_envs) if (e + call // 40) % 7 == 0], ext, cpe)
        if side and call == calls // 2:
            obs = reset_both()
        with torch.cuda.stream(stream):
            act = torch_driver(torch, obs, gen, dev)
            o, rew, te, tr, info = venv.step(act)
            got = [x.clone() for x in (o, rew, te, tr, info["final_obs"], info["state"], info["final_state"])]
        torch.cuda.synchronize()
        o, rew, te, tr, fo, st, fs = [x.cpu().numpy() for x in got]
        obs = got[0]
        want = host.call(act.cpu().numpy().astype(np.float64))
        at = f", call {call}"
        np.testing.assert_array_equal(te, want["terminated"], err_msg="terminated" + at)
        np.testing.assert_array_equal(tr, want["truncated"], err_msg="truncated" + at)
        np.testing.assert_array_equal(rew, want["reward"], err_msg="reward" + at)
        if want["final_obs"] is not None:
            np.testing.assert_array_equal(fo[want["ended"]], want["final_obs"], err_msg="final_obs" + at)
            np.testing.assert_array_equal(fs[want["ended"]], want["final_state"], err_msg="final_state" + at)
        np.testing.assert_array_equal(o, want["obs"], err_msg="obs" + at)
        np.testing.assert_array_equal(st, want["state"], err_msg="state" + at)
        np.add.at(off_term_of_track, A.track_of_env[want["terminated"] & want["off"].any(axis=1)], 1)
        off_streak = np.where(want["off"].any(axis=1), off_streak + 1, 0)
        term_streak = np.where(want["terminated"], term_streak + 1, 0)
        best_streak = [max(best_streak[0], int(off_streak.max())), max(best_streak[1], int(term_streak.max()))]
    _same_state(A, B)
    c = host.count
    print(f"counts {c}, off-track terminations per track {off_term_of_track.tolist()}, longest off-track / terminated run {best_streak}")
    for k in opt.get("need", []):
        assert c[k] > 0, (k, c)
    if opt.get("need_off_term_per_track"):
        assert (off_term_of_track > 0).all(), off_term_of_track
    if not AR:
        # nothing is reset: every env has made every step, the penalty was charged call after call, terminated stayed set
        np.testing.assert_array_equal(A.steps(), np.full(n_envs, calls * R))
        assert best_streak[0] >= 3 and best_streak[1] >= 3 and c["penalised"] > c["off_term"] > 0, (best_streak, c)
    print(f"twin ok: {calls} calls, kernel {A.kernel_name()}")
    venv.close()


def defaults(opt):
    """ftgp_step_device_ex(io, NULL) with default signals against ftgp_step_device on a twin DeviceVecEnv: every output, every call."""
    import torch
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    kw = dict(n_envs=64, n_rays=120, max_episode_steps=60, lap_target=1, spawn_mode=1, seed=7)
    track = load_track("small-circle")
    X, Y = DeviceVecEnv(track, **kw), DeviceVecEnv(track, **kw)
    dev = X.device
    paths = [np.asarray(track.path, dtype=np.float64)] * 64
    ex = X.env.lib.fn("step_device_ex")
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    obs = X.reset().clone()
    Y.reset()
    ends = 0
    for call in range(opt.get("calls", 200)):
        if call % 60 == 5:
            teleport([X.env, Y.env], paths, [e for e in range(64) if (e + call) % 5 == 0], [0], 1)
        act = torch_driver(torch, obs, gen, dev)
        X._check_actions(act)
        X._io.action, X._io.stream = act.data_ptr(), torch.cuda.current_stream(dev).cuda_stream
        X.env.lib.check(ex(X.env.h, X._io_ref, None))
        Y.step(act)
        torch.cuda.synchronize()
        for name in ("obs", "reward", "terminated", "truncated", "final_obs"):
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(Y, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        ends += int(X.terminated.sum()) + int(X.truncated.sum())
        obs = X.obs.clone()
    _same_state(X.env, Y.env)
    assert ends > 0
    X.close()
    Y.close()
    print(f"defaults ok: {ends} episode ends")


def errors(opt):
    import torch
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    track = load_track("small-circle")
    lib = capi.load()

    def refused(code, what, f, *a, **k):
        try:
            f(*a, **k)
        except capi.FtgpError as x:
            assert x.code == code, (what, x)
        else:
            raise AssertionError(f"{what} was accepted")

    with capi.Env(lib, track, n_envs=8, n_rays=64) as e:
        refused(-4, "signals before device_io_config", e.device_io_signals, 4, 5.0)
        buf = torch.zeros(8 * 8, device="cuda:0")
        refused(-4, "state_device before device_io_config", e.state_device, buf.data_ptr())
    # An obs allocation too small for n_beams.  The check knows an allocation's extent from the runtime, and torch carves small tensors
    # out of larger allocations: 12 MB is an allocation of its own.  1024 x 4096 rays in beams of 4 need 4 MB of it, raw rows 16 MB.
    with capi.Env(lib, track, n_envs=1024, n_rays=4096, spawn_mode=1, seed=7) as e:
        e.device_io_config(None, 100, 1, True)
        obs12, act = torch.zeros(3 << 20, device="cuda:0"), torch.ones((1024, 1, 2), device="cuda:0")
        rew, te, tr = (torch.zeros(1024, device="cuda:0") for _ in range(3))
        ptrs = [act.data_ptr(), obs12.data_ptr(), rew.data_ptr(), te.data_ptr(), tr.data_ptr()]
        refused(-1, "an obs allocation too small for n_rays", e.step_device, *ptrs)
        e.device_io_signals(1, 5.0)
        refused(-1, "an obs allocation too small for n_beams", e.step_device, *ptrs)
        e.device_io_signals(4, 5.0)
        e.step_device(*ptrs)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(obs12[:1024 * 1024].cpu().numpy().reshape(1024, 1024), sm.pool_scan(e.lidar(), 4, 5.0))
        assert not obs12[1024 * 1024:].any().item()
        del obs12
    venv = DeviceVecEnv(track, n_envs=8, n_rays=64, max_episode_steps=100, scan_pool=4, scan_max_range=5.0, state=True)
    E = venv.env
    for what, args in (("pool 0", (0,)), ("pool -2", (-2,)), ("pool 7 of 64 rays", (7,)), ("pool 128 of 64 rays", (128,)),
                       ("a negative max range", (4, -1.0)), ("a NaN max range", (4, float("nan"))), ("an infinite max range", (4, float("inf"))),
                       ("a negative penalty", (4, 5.0, False, -0.5)), ("a NaN penalty", (4, 5.0, False, float("nan"))),
                       ("an infinite penalty", (4, 5.0, False, float("inf")))):
        refused(-1, what, E.device_io_signals, *args)
    venv.reset()
    act = torch.ones((8, 1, 2), device="cuda:0")
    for _ in range(3):
        venv.step(act)
    torch.cuda.synchronize()

    def snapshot():
        return (E.steps(), E.pose(), E.progress(), E.lidar(), venv.obs.cpu().numpy(), venv.state.cpu().numpy())
    before = snapshot()
    ptrs = [act.data_ptr(), venv.obs.data_ptr(), venv.reward.data_ptr(), venv.terminated.data_ptr(), venv.truncated.data_ptr()]
    host = np.zeros((8, 1, 8), dtype=np.float32)
    refused(-1, "a host pointer for state", E.step_device, *ptrs, state=host.ctypes.data)
    refused(-1, "a host pointer for final_state", E.step_device, *ptrs, state=venv.state.data_ptr(), final_state=host.ctypes.data)
    refused(-1, "a host pointer for ftgp_state_device", E.state_device, host.ctypes.data)
    torch.cuda.synchronize()
    for x, y in zip(before, snapshot()):          # nothing was enqueued by a refused call
        np.testing.assert_array_equal(x, y)
    venv.step(act)
    torch.cuda.synchronize()
    assert venv.obs.max().item() <= 1.0 and venv.state[:, 0, 3].cpu().numpy().tolist() == [1.0] * 8
    # ftgp_device_io_config again: the defaults are back -- the call wants rows of n_rays floats again, and writes raw ranges
    E.device_io_config(None, 100, 1, True)
    full = torch.zeros((8, 1, 64), device="cuda:0")
    ptrs[1] = full.data_ptr()
    E.step_device(*ptrs)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(full.cpu().numpy().reshape(8, 64), E.lidar())
    assert full.max().item() > 1.0
    venv.close()
    print("errors ok")


SCENARIOS = {"twin": twin, "defaults": defaults, "errors": errors}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
