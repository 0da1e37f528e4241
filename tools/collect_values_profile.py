"""What values cost a collected rollout, one row per run:

    python tools/collect_values_profile.py --mode plain|values|torch [--envs 4096] [--rays 1080] [--decisions 32] [--calls 12]
                                           [--track track] [--lib PATH] [--out FILE]

plain   DeviceVecEnv.collect(T, noise=True) -- ftgp_collect_device as before.  With --lib, the library of another build (one that
        lacks the value entries too: this mode uses none of them) stands in for ft_grandprix_amd/lib/libftgp.so, so that the same
        file times the parent commit's plain collect beside this tree's.
values  collect(T, noise=True, values=True): value, next_value, advantage and returns from the device.
torch   what a learner does without the value entries: collect(T, noise=True, next_inputs=True), then the same critic as an
        nn.Sequential over inputs and over next_inputs ([T * N, n_in] each, no gradient) and the advantage recursion as a loop of T
        iterations of small torch kernels.

The policy is a random 85 -> 64 -> 64 -> 2 tanh MLP on beams 14 .. 93 of pool 10 and the five state inputs (at another --rays: the beams
of the scan window), the critic 85 -> 64 -> 64 -> 1.  One warm-up call, then --calls calls into one Rollout (out=); per-call time from
HIP events on torch's stream.  Prints one JSON line (median, minimum, maximum and every call's milliseconds, the kernel sources'
hash) and appends it to --out.  Run it in a fresh process: torch is imported first (ft_grandprix_amd/vec.py).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before libftgp.so)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi, net  # noqa: E402
from evidence import sha  # noqa: E402


def mlp(n_in, n_out, last):
    layers = [torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, n_out)]
    return torch.nn.Sequential(*(layers + ([torch.nn.Tanh()] if last else [])))


def torch_gae(reward, value, next_value, terminated, truncated, gamma, lam):
    T = reward.shape[0]
    adv = torch.empty_like(reward)
    a = torch.zeros_like(reward[0])
    for t in range(T - 1, -1, -1):
        live = (~terminated[t]).to(reward.dtype)[:, None]
        cont = (~(terminated[t] | truncated[t])).to(reward.dtype)[:, None]
        delta = reward[t] + gamma * live * next_value[t] - value[t]
        a = delta + gamma * lam * cont * a
        adv[t] = a
    return adv, adv + value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("plain", "values", "torch"), required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--decisions", type=int, default=32)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--track", default="track")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        capi._product = capi.CLib(os.path.abspath(a.lib), "ftgp_")
    from ft_grandprix_amd.vec import DeviceVecEnv
    eighth = int(a.rays / 8.0)
    first = -(-eighth // a.pool)
    n_beams = (a.rays - eighth) // a.pool - first
    n_in = n_beams + 5
    torch.manual_seed(0)
    policy, critic = mlp(n_in, 2, True), mlp(n_in, 1, False)
    spec = net.from_torch(policy, pool=a.pool, max_range=10.0, beam_first=first, n_beams=n_beams, use_state=True, out_scale=(2.0, 0.6), out_offset=(2.5, 0.0))
    env = DeviceVecEnv(a.track, n_envs=a.envs, n_rays=a.rays, roster=["agent"], nets={0: spec}, max_episode_steps=200, spawn_mode=1, seed=7)
    env.reset()
    T, gamma, lam = a.decisions, 0.99, 0.95
    kw = dict(std=(0.3, 0.1), clip=((0.0, 6.0), (-0.6, 0.6)), noise=True)
    if a.mode == "values":
        env.set_value_net(0, critic)
    critic = critic.to(env.device)

    def call(roll):
        if a.mode == "plain":
            return env.collect(T, out=roll, **kw)
        if a.mode == "values":
            return env.collect(T, out=roll, values=True, gamma=gamma, lam=lam, **kw)
        roll = env.collect(T, out=roll, next_inputs=True, **kw)
        with torch.no_grad():
            value = critic(roll.inputs.reshape(-1, n_in)).reshape(roll.reward.shape)
            next_value = critic(roll.next_inputs.reshape(-1, n_in)).reshape(roll.reward.shape)
            roll.advantage, roll.returns = torch_gae(roll.reward, value, next_value, roll.terminated, roll.truncated, gamma, lam)
        roll.value, roll.next_value = value, next_value
        return roll

    roll = call(None)
    if a.mode == "torch":
        roll.value = roll.next_value = roll.advantage = roll.returns = None      # (out= takes the c buffers alone)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if a.mode == "torch":
            roll.value = roll.next_value = roll.advantage = roll.returns = None
        e0.record()
        roll = call(roll)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    row = {"row": "collect " + a.mode, "lib": a.lib or "tree", "envs": a.envs, "rays": a.rays, "decisions": T, "calls": a.calls,
           "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "ms": [round(x, 3) for x in ms],
           "us_per_decision": 1e3 * float(np.median(ms)) / T, "env_steps_per_s": a.envs * T / (1e-3 * float(np.median(ms))),
           "ends": int((roll.terminated | roll.truncated).sum()), "kernel_source_sha": sha()}
    if a.mode != "plain":
        row["advantage_abs_mean"] = float(roll.advantage.abs().mean())
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
