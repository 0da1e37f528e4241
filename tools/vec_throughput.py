"""Env-steps/s of the device I/O loop (DeviceVecEnv.step on torch tensors) against the host loop (set_ctrl + step + get_lidar).

    python tools/vec_throughput.py [--envs 4096] [--rays 1080] [--calls 200] [--warmup 20] [--track track] [--rows device,torch_pool,signals,contacts,frame,rivals,host] [--repeats 1,4] [--cars 1]
                                   [--max-episode-steps 3000] [--random-start] [--dynamics]

Device loop: constant actions, and random torch actions drawn before every call, at action_repeat 1 and 4; per-call time from HIP
events on torch's stream around the timed calls.  Pooled observations (action_repeat 1, constant actions, beams of --pool rays clipped
at --max-range and scaled): "torch_pool" = the raw scan plus the torch ops a user would write (-1 -> M, clamp, reshape(...).amin(-1),
scale), "signals" = the same from the library (scan_pool, scan_max_range, state=True: ftgp_io_finish_signals_kernel), "contacts" = the
signals row with contact rows, both contact terminations and both penalties on top (ftgp_io_contact_kernel between the step and the
finish kernel), "frame" = the raw scan with the track frame on top (lookahead=8, dense_progress=True: ftgp_io_frame_kernel before and
after the steps, rows and reward by ftgp_io_finish_signals_kernel), "rivals" = the frame row with the rival rows on top (rivals=True,
n_rivals=3: ftgp_io_rival_kernel behind the frame kernel; meaningful with --cars 4, and its difference to the frame row is what the
channel costs).  --cars: cars per env, every one an agent.  --random-start: the device rows run under a spawn rule (ftgp_set_spawn_rule:
lateral share 0.8, yaw offsets up to 0.2 rad, shuffled grid); with a small --max-episode-steps the auto-reset, and with it the draw, runs often.
--dynamics: the device rows run with the per-car dynamics table on (randomize_dynamics: friction 0.3 .. 0.9, mass 4 .. 8 kg; the step
kernel's DYN form, and a fresh draw for the envs that ended after every call); the row without the switch is what it is compared with.
Host loop: per
step set_ctrl (one copy + synchronisation), step(1), get_lidar (the whole scan back).  One JSON line per row, then a summary line.  Run it in a fresh process: torch is imported first
(ft_grandprix_amd/vec.py).  Under `rocprofv3 --kernel-trace --stats -- python tools/vec_throughput.py` the per-kernel times of a call
(ftgp_io_ingest_kernel, ftgp_step_kernel, ftgp_io_contact_kernel, ftgp_io_finish_kernel / ftgp_io_finish_signals_kernel) come out of
the stats file.
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


def device_row(track, a, repeat, actions, pooled=None):
    """pooled: None = the raw scan; "torch" = pooled, clipped and scaled with torch ops after the call; "signals" = by the library;
    "contacts" = signals and the contact signals; "frame" = the raw scan, frame rows with 8 look-ahead points and the dense reward; "rivals" = frame and rival rows with 3 mate slots."""
    kw = dict(scan_pool=a.pool, scan_max_range=a.max_range, state=True) if pooled in ("signals", "contacts") else {}
    if pooled == "contacts":
        kw.update(contacts=True, terminate_on_wall_contact=True, terminate_on_car_contact=True, wall_contact_penalty=1.0, car_contact_penalty=0.5)
    if pooled in ("frame", "rivals"):
        kw.update(lookahead=8, dense_progress=True)
    if pooled == "rivals":
        kw.update(rivals=True, n_rivals=3)
    if a.random_start:
        kw.update(random_start=True, start_lateral=0.8, start_yaw_jitter=0.2, shuffle_grid=True)
    if a.dynamics:
        kw.update(randomize_dynamics={"friction": (0.3, 0.9), "mass": (4.0, 8.0)}, dynamics_seed=3)
    venv = DeviceVecEnv(track, n_envs=a.envs, n_rays=a.rays, cars_per_env=a.cars, max_episode_steps=a.max_episode_steps, action_repeat=repeat, spawn_mode=1,
                        seed=7, **kw)
    dev = venv.device
    M, inv = float(a.max_range), 1.0 / float(a.max_range)

    def step(actions_):
        obs = venv.step(actions_)[0]
        if pooled == "torch":
            obs = torch.where(obs < 0, M, obs).clamp(max=M).reshape(a.envs, a.cars, a.rays // a.pool, a.pool).amin(-1) * inv
        return obs

    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    const = torch.tensor([1.5, 0.0], device=dev).expand(a.envs, a.cars, 2).contiguous()

    def act():
        if actions == "constant":
            return const
        u = torch.rand((a.envs, a.cars, 2), generator=gen, device=dev)
        return torch.stack([3.0 * u[..., 0], 2.0 * u[..., 1] - 1.0], dim=2)

    venv.reset()
    for _ in range(a.warmup):
        step(act())
    stream = torch.cuda.current_stream(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    w0 = time.perf_counter()
    for _ in range(a.calls):
        step(act())
    t1.record(stream)
    t1.synchronize()
    wall = time.perf_counter() - w0
    ms = t0.elapsed_time(t1)
    step_ms = venv.env.last_kernel_ms()
    kernel = venv.env.kernel_name()
    episodes = int(venv.episode_index().sum()) if a.random_start else None
    venv.close()
    loop = {None: "device", "torch": "device+torch_pool", "signals": "device+signals", "contacts": "device+signals+contacts", "frame": "device+frame",
            "rivals": "device+frame+rivals"}[pooled]
    extra = {} if pooled in (None, "frame", "rivals") else {"pool": a.pool, "max_range": a.max_range}
    extra["max_episode_steps"] = a.max_episode_steps
    if a.random_start:
        extra.update(random_start=True, resets=episodes)
    if a.dynamics:
        extra.update(dynamics=True, step_kernel=kernel)
    return {"loop": loop, "actions": actions, "action_repeat": repeat, "envs": a.envs, "cars": a.cars, "rays": a.rays, "calls": a.calls, **extra,
            "us_per_call": 1e3 * ms / a.calls, "host_us_per_call": 1e6 * wall / a.calls, "step_kernel_us_last_call": 1e3 * step_ms,
            "env_steps_per_s": a.envs * repeat * a.calls / (ms * 1e-3)}


def host_row(track, a):
    lib = capi.load()
    n = max(10, a.calls // 4)
    with capi.Env(lib, track, n_envs=a.envs, cars_per_env=a.cars, n_rays=a.rays, spawn_mode=1, seed=7) as e:
        ctrl = np.tile(np.array([1.5, 0.0]), (a.envs * a.cars, 1))
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
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--max-range", type=float, default=10.0)
    ap.add_argument("--repeats", default="1,4", help="action_repeat of the device rows, comma-separated")
    ap.add_argument("--cars", type=int, default=1, help="cars per env, every one an agent")
    ap.add_argument("--max-episode-steps", type=int, default=3000, help="truncation of the device rows")
    ap.add_argument("--random-start", action="store_true", help="the device rows run under a spawn rule")
    ap.add_argument("--dynamics", action="store_true", help="the device rows run with the per-car dynamics table on (randomize_dynamics)")
    ap.add_argument("--rows", default="device,torch_pool,signals,host", help="comma-separated: device, torch_pool, signals, contacts, frame, rivals, host")
    a = ap.parse_args()
    want = set(a.rows.split(","))
    track = load_track(a.track)
    rows = []
    if "device" in want:
        for repeat in (int(r) for r in a.repeats.split(",")):
            for actions in ("constant", "random"):
                rows.append(device_row(track, a, repeat, actions))
                print(json.dumps(rows[-1]), flush=True)
    for name, pooled in (("torch_pool", "torch"), ("signals", "signals"), ("contacts", "contacts"), ("frame", "frame"), ("rivals", "rivals")):
        if name in want:
            rows.append(device_row(track, a, 1, "constant", pooled))
            print(json.dumps(rows[-1]), flush=True)
    if "host" in want:
        rows.append(host_row(track, a))
        print(json.dumps(rows[-1]), flush=True)
        host = rows[-1]["env_steps_per_s"]
        print(json.dumps({"summary": {f"device_r{r['action_repeat']}_{r['actions']}_over_host": r["env_steps_per_s"] / host
                                      for r in rows if r["loop"] == "device"}}))


if __name__ == "__main__":
    main()
