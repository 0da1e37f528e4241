"""What saving, restoring and forking env states costs (ftgp_save_envs_device / ftgp_load_envs_device, DeviceVecEnv.fork), against a
torch device-to-device copy of the same number of bytes timed in the same run.

    python tools/env_state_throughput.py [--envs 4096] [--rays 1080] [--cars 1,4] [--calls 41] [--warmup 10] [--track track]

Per cars-per-env one DeviceVecEnv, driven 50 calls so that the state is not the spawn state.  Every row is the median over --calls
(>= 31) calls, each between its own pair of HIP events on torch's stream, after --warmup calls:
  copy           dst.copy_(src) of two uint8 tensors of n_envs * bytes_per_env bytes: the yardstick
  fences         ftgp_state_device, a kernel of one lane per car that writes 32 bytes each, ordered on torch's stream the way save and
                 load are (an event on torch's stream, a wait on the handle's, the kernel, an event there, a wait on torch's): what
                 every such entry costs before it moves a byte
  save           ftgp_save_envs_device, all envs
  load           ftgp_load_envs_device, row e -> env e
  fork_one       save, then load with src_row = 0 for every env
  fork_perm      save, then load with a random permutation
  vec_fork_one / vec_fork_perm   DeviceVecEnv.fork(src): the two library calls, torch's int64 -> int32 of src and ftgp_obs_device
  step           DeviceVecEnv.step with constant actions, for scale: what a fork per planning step adds to
One JSON line per row; "copy_rate_ratio" = the row's bytes per second over the copy's (save and load move the same bytes as the copy,
a fork twice as many: its ratio counts both passes).  Run it in a fresh process: torch is imported first (ft_grandprix_amd/vec.py).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libftgp.so)

from ft_grandprix_amd.track import load_track  # noqa: E402
from ft_grandprix_amd.vec import DeviceVecEnv  # noqa: E402


def median_us(fn, stream, calls, warmup):
    for _ in range(warmup):
        fn()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for t0, t1 in events:
        t0.record(stream)
        fn()
        t1.record(stream)
    events[-1][1].synchronize()
    return 1e3 * statistics.median(t0.elapsed_time(t1) for t0, t1 in events)


def rows_of(track, a, cars):
    venv = DeviceVecEnv(track, n_envs=a.envs, n_rays=a.rays, cars_per_env=cars, max_episode_steps=3000, spawn_mode=1, seed=7)
    dev, env, n = venv.device, venv.env, a.envs
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    act = torch.tensor([1.5, 0.0], device=dev).expand(n, cars, 2).contiguous()
    venv.reset()
    for _ in range(50):
        venv.step(act)
    bpe = venv.bytes_per_env
    buf, other = (torch.zeros((n, bpe), dtype=torch.uint8, device=dev) for _ in range(2))
    one = torch.zeros(n, dtype=torch.int32, device=dev)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    perm32 = perm.to(torch.int32)
    env.save_envs_device(buf.data_ptr(), n, 0, s)

    def fork(src):
        env.save_envs_device(buf.data_ptr(), n, 0, s)
        env.load_envs_device(buf.data_ptr(), n, src.data_ptr(), s)

    state = torch.zeros((n, cars, 8), dtype=torch.float32, device=dev)
    cases = (("copy", 1, lambda: other.copy_(buf)),
             ("fences", 0, lambda: env.state_device(state.data_ptr(), s)),
             ("save", 1, lambda: env.save_envs_device(buf.data_ptr(), n, 0, s)),
             ("load", 1, lambda: env.load_envs_device(buf.data_ptr(), n, 0, s)),
             ("fork_one", 2, lambda: fork(one)),
             ("fork_perm", 2, lambda: fork(perm32)),
             ("vec_fork_one", 2, lambda: venv.fork(one)),
             ("vec_fork_perm", 2, lambda: venv.fork(perm)),
             ("step", 0, lambda: venv.step(act)))
    out, copy_us = [], None
    for name, passes, fn in cases:
        us = median_us(fn, stream, a.calls, a.warmup)
        copy_us = us if name == "copy" else copy_us
        row = {"row": name, "envs": n, "cars": cars, "rays": a.rays, "bytes_per_env": bpe, "calls": a.calls, "us_per_call": us}
        if passes:
            row["gb_per_s_moved"] = 2 * passes * n * bpe / (us * 1e-6) / 1e9        # read and written
            row["copy_rate_ratio"] = passes * copy_us / us
        out.append(row)
        print(json.dumps(row), flush=True)
    assert env.env_state_rejected() == 0
    venv.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--cars", default="1,4", help="cars per env, comma-separated; every one an agent")
    ap.add_argument("--calls", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--track", default="track")
    a = ap.parse_args()
    if a.calls < 31:
        ap.error("--calls: at least 31 timed calls")
    track = load_track(a.track)
    for cars in (int(c) for c in a.cars.split(",")):
        rows_of(track, a, cars)


if __name__ == "__main__":
    main()
