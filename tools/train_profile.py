"""What the update of a PPO iteration costs, one row per run:

    python tools/train_profile.py --mode device|torch [--envs 1024] [--rays 1080] [--decisions 32] [--iterations 12]
                                  [--epochs 4] [--minibatches 4] [--track track] [--out FILE]

device  DeviceVecEnv.ppo_update on a collect(values=True) rollout: per minibatch one ftgp_train_grad_device and one
        ftgp_train_adam_device on the slot's parameters in place.
torch   the update of tools/ppo.py's default path: torch autograd on the clipped surrogate and the squared value error, Adam, then
        set_net_params and set_value_params.

The policy is a random 85 -> 64 -> 64 -> 2 tanh MLP on beams 14 .. 93 of pool 10 and the five state inputs, the critic
85 -> 64 -> 64 -> 1.  Every iteration collects a rollout (not timed) and times its update by HIP events on torch's stream; one warm-up
iteration.  Prints one JSON line (median, minimum, maximum and every update's milliseconds, the kernel sources' hash) and appends it to
--out.  Run it in a fresh process: torch is imported first (ft_grandprix_amd/vec.py).
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

from ft_grandprix_amd import net  # noqa: E402
from evidence import sha  # noqa: E402


def mlp(n_in, n_out, last):
    layers = [torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, n_out)]
    return torch.nn.Sequential(*(layers + ([torch.nn.Tanh()] if last else [])))


def flat(module):
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("device", "torch"), required=True)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--decisions", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=12)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--track", default="track")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ft_grandprix_amd.vec import DeviceVecEnv
    eighth = int(a.rays / 8.0)
    first = -(-eighth // a.pool)
    n_beams = (a.rays - eighth) // a.pool - first
    n_in = n_beams + 5
    torch.manual_seed(0)
    policy, critic = mlp(n_in, 2, True), mlp(n_in, 1, False)
    fields = dict(pool=a.pool, max_range=10.0, beam_first=first, n_beams=n_beams, use_state=True, out_scale=(2.0, 0.6), out_offset=(2.5, 0.0))
    env = DeviceVecEnv(a.track, n_envs=a.envs, n_rays=a.rays, roster=["agent"], nets={0: net.from_torch(policy, **fields)},
                       max_episode_steps=200, spawn_mode=1, seed=7)
    env.set_value_net(0, critic)
    env.reset()
    dev = env.device
    policy, critic = policy.to(dev), critic.to(dev)
    scale, offset = torch.tensor(fields["out_scale"], device=dev), torch.tensor(fields["out_offset"], device=dev)
    std_t = (0.3, 0.1)
    std = torch.tensor(std_t, device=dev)
    lr, clip = 3e-4, 0.2
    if a.mode == "device":
        env.train_begin(0)
    opt = torch.optim.Adam(list(policy.parameters()) + list(critic.parameters()), lr=lr)
    T = a.decisions

    def update(roll):
        if a.mode == "device":
            return env.ppo_update(roll, 0, epochs=a.epochs, minibatches=a.minibatches, lr=lr, clip=clip, value_coef=0.5, std=std_t)[-1, 2]
        x = roll.inputs.reshape(-1, n_in)
        z = roll.noise.reshape(-1, 2)
        proposed = roll.mean.reshape(-1, 2) + std * z
        old_logp = (-0.5 * z * z).sum(dim=1)
        adv, ret = roll.advantage.reshape(-1), roll.returns.reshape(-1)
        for _ in range(a.epochs):
            for idx in torch.randperm(x.shape[0], device=dev).chunk(a.minibatches):
                mean = policy(x[idx]) * scale + offset
                logp = (-0.5 * ((proposed[idx] - mean) / std) ** 2).sum(dim=1)
                ratio = torch.exp(logp - old_logp[idx])
                ad = adv[idx]
                ad = (ad - ad.mean()) / (ad.std() + 1e-8)
                loss_pi = -torch.min(ratio * ad, ratio.clamp(1.0 - clip, 1.0 + clip) * ad).mean()
                loss_v = 0.5 * ((critic(x[idx]).squeeze(1) - ret[idx]) ** 2).mean()
                opt.zero_grad(set_to_none=True)
                (loss_pi + 0.5 * loss_v).backward()
                opt.step()
        env.set_net_params(0, flat(policy))
        env.set_value_params(0, flat(critic))
        return loss_v.detach()

    roll, ms, loss_v = None, [], None
    for it in range(a.iterations + 1):
        roll = env.collect(T, std=std_t, clip=((0.0, 6.0), (-0.6, 0.6)), noise=True, values=True, out=roll)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss_v = update(roll)
        e1.record()
        e1.synchronize()
        if it > 0:
            ms.append(e0.elapsed_time(e1))
    row = {"row": "update " + a.mode, "envs": a.envs, "rays": a.rays, "decisions": T, "epochs": a.epochs, "minibatches": a.minibatches,
           "rows": a.envs * T, "iterations": a.iterations, "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
           "ms": [round(x, 3) for x in ms], "loss_v": float(loss_v), "kernel_source_sha": sha()}
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
