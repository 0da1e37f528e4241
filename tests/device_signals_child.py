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
from tests.device_twin import HostTwin, _same_state, _tracks, push_off, refused, teleport, torch_driver  # noqa: E402


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
