"""Child process of tests/test_device_io.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/device_io_child.py <scenario> [json options]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def guard(order):
    """The runtime guard (no device is touched): order "torch_first" must pass with one runtime mapped, "lib_first" must raise."""
    if order == "torch_first":
        import torch  # noqa: F401
        from ft_grandprix_amd import capi, vec
        capi.load()
        vec.check_single_hip_runtime()
        rt = vec.mapped_hip_runtimes()
        assert len(rt["libamdhip64"]) == 1, rt
        print("guard passed:", rt)
    else:
        from ft_grandprix_amd import capi
        capi.load()
        import torch  # noqa: F401
        from ft_grandprix_amd import vec
        try:
            vec.check_single_hip_runtime()
        except RuntimeError as e:
            assert vec.RUNTIME_ERROR in str(e), e
            print("guard raised:", e)
            return
        raise AssertionError(f"the guard passed with {vec.mapped_hip_runtimes()}")


# ------------------------------------------------------------------------------------------------------------------ GPU scenarios
def twin(opt):
    """DeviceVecEnv (handle A) against the host path (twin B), bit for bit, every call."""
    import torch
    import numpy as np
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    from tests.device_twin import teleport

    n_envs, n_rays, cpe = opt.get("n_envs", 256), opt.get("n_rays", 1080), opt.get("cars_per_env", 1)
    roster = opt.get("roster", ["agent"] * cpe)
    R, M, AR = opt.get("action_repeat", 1), opt.get("max_episode_steps", 700), opt.get("auto_reset", True)
    calls, side = opt.get("calls", 1500), opt.get("side_stream", False)
    kw = dict(lap_target=1, spawn_mode=1, seed=7, lidar_mode=opt.get("lidar_mode", "rangefinder"))
    track = load_track(opt.get("track", "small-circle"))
    paths = [np.asarray(track.path, dtype=np.float64)] * n_envs
    dev = torch.device("cuda", 0)
    venv = DeviceVecEnv(track, n_envs=n_envs, n_rays=n_rays, cars_per_env=cpe, roster=roster, max_episode_steps=M,
                        action_repeat=R, auto_reset=AR, device_id=0, **kw)
    B = capi.Env(capi.load(), track, n_envs=n_envs, cars_per_env=cpe, n_rays=n_rays, **kw)
    ext = [k for k, r in enumerate(roster) if r == "agent"]
    bundled = len(ext) < cpe
    if bundled:
        B.set_car_policies(["lobotomy" if r == "agent" else r for r in roster])
    car_mask = np.zeros((n_envs, cpe), dtype=np.uint8)
    car_mask[:, ext] = 1
    obs = venv.reset().clone()
    B.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(opt.get("seed", 1))
    stream = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)
    n_term = n_trunc = 0
    for call in range(calls):
        if call % 60 == 5:                        # bring some envs to the end of their lap: terminations
            teleport([venv.env, B], paths, [e for e in range(n_envs) if (e + call) % 5 == 0], ext, cpe, rolling=False)
        with torch.cuda.stream(stream):
            # a torch driver: steer towards the longest range of the front half, speed ~ U(0.5, 3); then noise, some of it past the
            # ctrlrange (speed, steer)
            front = obs[:, :, n_rays // 4: 3 * n_rays // 4]
            j = front.argmax(dim=2).float() / max(1, front.shape[2] - 1)
            steer = (j - 0.5) * 2.0
            speed = 0.5 + 2.5 * torch.rand((n_envs, len(ext)), generator=gen, device=dev)
            act = torch.stack([speed, steer + 0.3 * torch.randn((n_envs, len(ext)), generator=gen, device=dev)], dim=2)
            wild = torch.rand((n_envs, len(ext), 2), generator=gen, device=dev) < 0.05
            act = torch.where(wild, 6.0 * torch.randn((n_envs, len(ext), 2), generator=gen, device=dev), act).contiguous()
            o, rew, te, tr, info = venv.step(act)
            got = [x.clone() for x in (o, rew, te, tr, info["final_obs"])]
        torch.cuda.synchronize()
        o, rew, te, tr, fo = [x.cpu().numpy() for x in got]
        a = act.cpu().numpy().astype(np.float64)
        obs = got[0]
        # twin B: the host path
        p0 = B.progress()
        for _ in range(R):
            fin = B.progress()[:, 4].reshape(n_envs, cpe)
            ctrl = np.zeros((n_envs, cpe, 2), dtype=np.float64)
            if bundled:
                ctrl = B.policy_eval("per_car", B.lidar()).reshape(n_envs, cpe, 2)
            ctrl[:, ext] = np.where(fin[:, ext, None] != 0, 0.0, a)
            B.set_ctrl(ctrl, car_mask if bundled else None)
            B.step(1)
        p1 = B.progress()
        reward = (p1[:, 3] - p0[:, 3]).reshape(n_envs, cpe)[:, ext].astype(np.float32)
        term = (p1[:, 4].reshape(n_envs, cpe)[:, ext] != 0).all(axis=1)
        trunc = ~term & (M > 0) & (B.steps() >= M)
        lid = B.lidar().reshape(n_envs, cpe, n_rays)[:, ext]
        ended = term | trunc
        np.testing.assert_array_equal(te, term, err_msg=f"terminated, call {call}")
        np.testing.assert_array_equal(tr, trunc, err_msg=f"truncated, call {call}")
        np.testing.assert_array_equal(rew, reward, err_msg=f"reward, call {call}")
        if AR and ended.any():
            np.testing.assert_array_equal(fo[ended], lid[ended], err_msg=f"final_obs, call {call}")
            B.reset(ended.astype(np.uint8))
            lid[ended] = 0.0
        np.testing.assert_array_equal(o, lid, err_msg=f"obs, call {call}")
        n_term += int(term.sum())
        n_trunc += int(trunc.sum())
    A = venv.env
    np.testing.assert_array_equal(A.pose(), B.pose())
    np.testing.assert_array_equal(A.progress(), B.progress())
    for x, y in zip(A.lap_times(), B.lap_times()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(A.steps(), B.steps())
    np.testing.assert_array_equal(A.lidar(), B.lidar())
    if opt.get("need_ends", True):
        assert n_term > 0 and n_trunc > 0, (n_term, n_trunc)
    if not AR:
        assert A.steps().max() > M, A.steps().max()
    print(f"twin ok: {calls} calls, {n_term} terminations, {n_trunc} truncations, kernel {A.kernel_name()}")
    venv.close()


def shared_roster(opt):
    """set_car_policies(X), device-io calls with roster Y, then the user's roster must be the one that runs."""
    import torch
    import numpy as np
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    X, Y = ["nidc", "fast", "random"], ["lobotomy", "agent", "nidc"]
    kw = dict(n_envs=64, n_rays=1080, cars_per_env=3, lap_target=1, spawn_mode=1, seed=11)
    track = load_track("small-circle")
    venv = DeviceVecEnv(track, roster=Y, max_episode_steps=40, action_repeat=2, **kw)
    A = venv.env
    B = capi.Env(capi.load(), track, **kw)
    A.set_car_policies(X)
    B.set_car_policies(X)
    venv.reset()
    act = torch.full((64, 1, 2), 1.5, device="cuda:0")
    for _ in range(30):
        venv.step(act)
    torch.cuda.synchronize()
    assert A.steps().max() > 0
    A.reset()                                   # the same state as B's: spawn, steps 0
    scans = np.random.default_rng(3).uniform(0.1, 5.0, (64 * 3, 1080)).astype(np.float32)
    np.testing.assert_array_equal(A.policy_eval("per_car", scans), B.policy_eval("per_car", scans))
    A.reset()
    B.reset()
    A.rollout("per_car", 50)
    B.rollout("per_car", 50)
    np.testing.assert_array_equal(A.pose(), B.pose())
    np.testing.assert_array_equal(A.progress(), B.progress())
    np.testing.assert_array_equal(A.ctrl(), B.ctrl())
    np.testing.assert_array_equal(A.lidar(), B.lidar())
    # and back: device-io calls after the user's rollout run roster Y again (the twin's own table is never touched)
    venv.step(act)
    torch.cuda.synchronize()
    venv.close()
    print("shared roster ok")


def errors(opt):
    import torch
    import numpy as np
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    track = load_track("small-circle")
    lib = capi.load()
    # ftgp_step_device before ftgp_device_io_config
    with capi.Env(lib, track, n_envs=8, n_rays=64) as e:
        buf = torch.zeros(8 * 64 + 64, device="cuda:0")
        p = buf.data_ptr()
        try:
            e.step_device(p, p, p, p, p)
        except capi.FtgpError as x:
            assert x.code == -4, x
        else:
            raise AssertionError("step_device before device_io_config was accepted")
    venv = DeviceVecEnv(track, n_envs=8, n_rays=64, max_episode_steps=100)
    venv.reset()
    act = torch.ones((8, 1, 2), device="cuda:0")
    for _ in range(3):
        venv.step(act)
    torch.cuda.synchronize()
    before = (venv.env.steps(), venv.env.pose(), venv.env.progress(), venv.env.lidar(), venv.obs.cpu().numpy())
    host = np.ones((8, 1, 2), dtype=np.float32)
    dev_ptrs = [venv.obs.data_ptr(), venv.reward.data_ptr(), venv.terminated.data_ptr(), venv.truncated.data_ptr()]
    for which in range(5):                      # a host address in each place in turn
        ptrs = [act.data_ptr()] + dev_ptrs
        ptrs[which] = host.ctypes.data
        try:
            venv.env.step_device(*ptrs)
        except capi.FtgpError as x:
            assert x.code == -1, x
        else:
            raise AssertionError(f"a host pointer in place {which} was accepted")
    torch.cuda.synchronize()
    after = (venv.env.steps(), venv.env.pose(), venv.env.progress(), venv.env.lidar(), venv.obs.cpu().numpy())
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    for bad in (act.double(), act.cpu(), act[:4], torch.ones((8, 2, 2), device="cuda:0"), act.transpose(0, 2).contiguous().transpose(0, 2)):
        try:
            venv.step(bad)
        except ValueError:
            pass
        else:
            raise AssertionError(f"DeviceVecEnv.step accepted {bad.dtype} {tuple(bad.shape)} on {bad.device}")
    venv.step(act)
    torch.cuda.synchronize()
    venv.close()
    print("errors ok")


SCENARIOS = {"twin": twin, "shared_roster": shared_roster, "errors": errors}

if __name__ == "__main__":
    name = sys.argv[1]
    opt = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    if name == "guard":
        guard(opt["order"])
    else:
        SCENARIOS[name](opt)
