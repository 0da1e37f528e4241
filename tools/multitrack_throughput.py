"""Env-steps/s of multi-track handles (ftgp_create_tracks) against the ways to race the same tracks without them.

    python tools/multitrack_throughput.py [--envs-per-track 1024] [--rays 1080] [--reps 5] [--calls 200]
    python tools/multitrack_throughput.py --trace      (a short, fixed sequence for rocprofv3 --kernel-trace --stats)

Rollout rows, the bundled fast driver on the device, launches of 20 and 500 steps, 4 x envs-per-track envs on track, circle,
small-circle and inkscape:
    tracks4_blocks / tracks4_xcd   one four-track handle, workgroups in block order / XCD-grouped order (FTGP_TRACK_ORDER)
    back_to_back                   four single-track handles, one launch each, issued one after the other, then all waited for
    single_<track>                 one single-track handle of all 4 x envs-per-track envs on that track
The time of a row is the wall time from the first launch to the end of the last (median of --reps), and, for one handle, the kernel
time of its launch (HIP events, ftgp_last_kernel_ms).  Device I/O rows: DeviceVecEnv.step calls per second with random torch actions,
four tracks (4 x envs-per-track envs) against one (the same number of envs on track), action_repeat 1 and 4.  One JSON line per row.
Run it in a fresh process: torch is imported before the library (ft_grandprix_amd/vec.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libftgp.so)

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402
from ft_grandprix_amd.vec import DeviceVecEnv  # noqa: E402

NAMES = ["track", "circle", "small-circle", "inkscape"]


def timed(handles, steps, reps):
    """Median wall time (s) of one launch of `steps` on every handle (issued back to back, then all waited for), and the kernel time
    of the last launch of each handle (s)."""
    for h in handles:
        h.rollout("fast", steps)
    for h in handles:
        h.last_kernel_ms()
    walls = []
    for _ in range(reps):
        w0 = time.perf_counter()
        for h in handles:
            h.rollout("fast", steps)
        for h in handles:
            h.last_kernel_ms()              # waits for the launch
        walls.append(time.perf_counter() - w0)
    return statistics.median(walls), [1e-3 * h.last_kernel_ms() for h in handles]


def rollout_rows(a):
    lib = capi.load()
    tracks = [load_track(n) for n in NAMES]
    n = a.envs_per_track
    kw = dict(n_rays=a.rays, spawn_mode=1, seed=7)
    variants = []
    for order in ("blocks", "xcd"):
        os.environ["FTGP_TRACK_ORDER"] = order
        variants.append((f"tracks4_{order}", [capi.Env(lib, tracks, n_envs=4 * n, envs_per_track=[n] * 4, **kw)]))
    os.environ.pop("FTGP_TRACK_ORDER", None)
    variants.append(("back_to_back", [capi.Env(lib, t, n_envs=n, env_base=k * n, **kw) for k, t in enumerate(tracks)]))
    for name, t in zip(NAMES, tracks):
        variants.append((f"single_{name}", [capi.Env(lib, t, n_envs=4 * n, **kw)]))
    for steps in (20, 500):
        for name, hs in variants:
            wall, kern = timed(hs, steps, a.reps)
            env_steps = 4 * n * steps
            row = {"row": name, "steps": steps, "envs": 4 * n, "rays": a.rays, "launches": len(hs), "wall_us_per_step": 1e6 * wall / steps,
                   "env_steps_per_s_wall": env_steps / wall}
            if len(hs) == 1:
                row["kernel_us_per_step"] = 1e6 * kern[0] / steps
                row["env_steps_per_s_kernel"] = env_steps / kern[0]
            else:
                row["kernel_us_per_step_sum"] = 1e6 * sum(kern) / steps
            print(json.dumps(row), flush=True)
    for _, hs in variants:
        for h in hs:
            h.close()


def vec_rows(a):
    n = a.envs_per_track
    for repeat in (1, 4):
        for name, track, kw in (("vec_tracks4", NAMES, dict(envs_per_track=[n] * 4)), ("vec_track1", "track", {})):
            venv = DeviceVecEnv(track, n_envs=4 * n, n_rays=a.rays, max_episode_steps=3000, action_repeat=repeat, spawn_mode=1, seed=7, **kw)
            dev = venv.device
            gen = torch.Generator(device=dev)
            gen.manual_seed(1)

            def act():
                u = torch.rand((4 * n, 1, 2), generator=gen, device=dev)
                return torch.stack([3.0 * u[..., 0], 2.0 * u[..., 1] - 1.0], dim=2)

            venv.reset()
            for _ in range(20):
                venv.step(act())
            stream = torch.cuda.current_stream(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            w0 = time.perf_counter()
            for _ in range(a.calls):
                venv.step(act())
            t1.record(stream)
            t1.synchronize()
            wall = time.perf_counter() - w0
            ms = t0.elapsed_time(t1)
            venv.close()
            print(json.dumps({"row": name, "action_repeat": repeat, "envs": 4 * n, "rays": a.rays, "calls": a.calls,
                              "calls_per_s": a.calls / (ms * 1e-3), "us_per_call": 1e3 * ms / a.calls, "host_us_per_call": 1e6 * wall / a.calls,
                              "env_steps_per_s": 4 * n * repeat * a.calls / (ms * 1e-3)}), flush=True)


def trace(a):
    """Three 20-step rollouts and five one-step device-I/O calls on a four-track handle: under rocprofv3 the trace shows one step
    launch per rollout and three launches per call."""
    lib = capi.load()
    tracks = [load_track(nm) for nm in NAMES]
    n = a.envs_per_track
    with capi.Env(lib, tracks, n_envs=4 * n, envs_per_track=[n] * 4, n_rays=a.rays, spawn_mode=1, seed=7) as e:
        for _ in range(3):
            e.rollout("fast", 20)
        e.last_kernel_ms()
    venv = DeviceVecEnv(NAMES, n_envs=4 * n, n_rays=a.rays, envs_per_track=[n] * 4, spawn_mode=1, seed=7)
    venv.reset()
    act = torch.zeros((4 * n, 1, 2), device=venv.device)
    for _ in range(5):
        venv.step(act)
    torch.cuda.synchronize()
    venv.close()
    print(json.dumps({"trace": "3 rollouts of 20 steps, 5 device-io calls", "envs": 4 * n}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs-per-track", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-vec", action="store_true")
    a = ap.parse_args()
    if a.trace:
        trace(a)
        return
    rollout_rows(a)
    if not a.no_vec:
        vec_rows(a)


if __name__ == "__main__":
    main()
