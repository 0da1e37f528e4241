"""Env-steps/s of the device I/O loop (DeviceVecEnv.step on torch tensors) against the host loop (set_ctrl + step + get_lidar).

    python tools/vec_throughput.py [--envs 4096] [--rays 1080] [--calls 200] [--warmup 20] [--track track]

Device loop: constant actions, and random torch actions drawn before every call, at action_repeat 1 and 4; per-call time from HIP
events on torch's stream around the timed calls.  Host loop: per step set_ctrl (one copy + synchronisation), step(1), get_lidar
(the whole scan back).  One JSON line per row, then a summary line.  Run it in a fresh process: torch is imported first
(ft_grandprix_amd/vec.py).  Under `rocprofv3 --kernel-trace --stats -- python tools/vec_throughput.py` the per-kernel times of a call
(ftgp_io_ingest_kernel, ftgp_step_kernel, ftgp_io_finish_kernel) come out of the stats file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libftgp.so)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402
from ft_grandprix_amd.vec import DeviceVecEnv  # noqa: E402


def device_row(track, a, repeat, actions):
    venv = DeviceVecEnv(track, n_envs=a.envs, n_rays=a.rays, max_episode_steps=3000, action_repeat=repeat, spawn_mode=1, seed=7)
    dev = venv.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    const = torch.tensor([1.5, 0.0], device=dev).expand(a.envs, 1, 2).contiguous()

    def act():
        if actions == "constant":
            return const
        u = torch.rand((a.envs, 1, 2), generator=gen, device=dev)
        return torch.stack([3.0 * u[..., 0], 2.0 * u[..., 1] - 1.0], dim=2)

    venv.reset()
    for _ in range(a.warmup):
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
    step_ms = venv.env.last_kernel_ms()
    venv.close()
    return {"loop": "device", "actions": actions, "action_repeat": repeat, "envs": a.envs, "rays": a.rays, "calls": a.calls,
            "us_per_call": 1e3 * ms / a.calls, "host_us_per_call": 1e6 * wall / a.calls, "step_kernel_us_last_call": 1e3 * step_ms,
            "env_steps_per_s": a.envs * repeat * a.calls / (ms * 1e-3)}


def host_row(track, a):
    lib = capi.load()
    n = max(10, a.calls // 4)
    with capi.Env(lib, track, n_envs=a.envs, n_rays=a.rays, spawn_mode=1, seed=7) as e:
        ctrl = np.tile(np.array([1.5, 0.0]), (a.envs, 1))
        for _ in range(5):
            e.set_ctrl(ctrl); e.step(1); e.lidar()
        w0 = time.perf_counter()
        for _ in range(n):
            e.set_ctrl(ctrl)
            e.step(1)
            e.lidar()
        wall = time.perf_counter() - w0
    return {"loop": "host", "actions": "constant", "action_repeat": 1, "envs": a.envs, "rays": a.rays, "calls": n,
            "us_per_call": 1e6 * wall / n, "env_steps_per_s": a.envs * n / wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--track", default="track")
    a = ap.parse_args()
    track = load_track(a.track)
    rows = []
    for repeat in (1, 4):
        for actions in ("constant", "random"):
            rows.append(device_row(track, a, repeat, actions))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(host_row(track, a))
    print(json.dumps(rows[-1]), flush=True)
    host = rows[-1]["env_steps_per_s"]
    print(json.dumps({"summary": {f"device_r{r['action_repeat']}_{r['actions']}_over_host": r["env_steps_per_s"] / host
                                  for r in rows if r["loop"] == "device"}}))


if __name__ == "__main__":
    main()
