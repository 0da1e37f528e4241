"""A minimal clipped-PPO loop on collected rollouts with values: the usage example of ftgp_set_value_net and ftgp_collect_values_device
(DeviceVecEnv.set_value_net, collect(values=True), set_net_params, set_value_params), in the shape of tools/evolve.py.

    python tools/ppo.py [--track circle] [--envs 1024] [--rays 1080] [--decisions 32] [--iterations 20] [--epochs 4] [--minibatches 4]
                        [--repeat 4] [--gamma 0.99] [--lam 0.95] [--clip 0.2] [--lr 3e-4] [--std 0.3,0.1] [--hidden 64] [--seed 0]
                        [--save policy.npz] [--device-update]

One DeviceVecEnv of --envs envs with one agent each; slot 0 holds the policy and its value net.  Per iteration:

    roll = env.collect(T, noise=True, values=True)        T decisions, the critic's values, the bootstrap values, advantages and
                                                          returns from the device -- nothing leaves it
    the action before the clip is mean + std * noise, so the behaviour policy's log-probability follows from roll.noise alone
    --epochs passes of --minibatches minibatches: torch autograd on roll.inputs with the clipped surrogate on roll.advantage (normalised
    per minibatch) and the squared error to roll.returns; Adam
    env.set_net_params(0, flat policy), env.set_value_params(0, flat critic)      the refresh, on torch's stream, no synchronisation

With --device-update the update never enters torch's autograd: env.train_begin(0) once, and per iteration env.ppo_update(roll, ...)
(ftgp_train_grad_device and ftgp_train_adam_device per minibatch, on the slot's parameters in place; one advantage normalisation over
the whole rollout instead of one per minibatch).  The torch path stays the default, and the comparison.

and one JSON line: the iteration, the mean reward per decision, the mean return, the losses, the seconds of the collect and of the
update.  torch's tanh differs from the library's in the seventh digit, so the ratio of the first minibatch is 1 to that precision.
No claim is made that this learns, or how fast: that depends on the settings, and nothing tests it.  Run it in a fresh process: torch
is imported first (ft_grandprix_amd/vec.py).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libftgp.so)

from ft_grandprix_amd import net  # noqa: E402
from ft_grandprix_amd.vec import DeviceVecEnv  # noqa: E402


def flat(module):
    """The parameters of an nn.Sequential of Linear layers in ftgp_set_net's flat layout: per layer W[n_out][n_in], then b[n_out]."""
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--track", default="circle")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--decisions", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=4, help="physics steps per decision (action_repeat)")
    ap.add_argument("--episode", type=int, default=2000, help="max_episode_steps")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--std", default="0.3,0.1")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="write the policy of the last iteration as an .npz (net.load reads it)")
    ap.add_argument("--device-update", action="store_true", help="the update on the device (DeviceVecEnv.ppo_update) instead of torch autograd + Adam")
    a = ap.parse_args()
    eighth = int(a.rays / 8.0)
    first = -(-eighth // a.pool)
    n_beams = (a.rays - eighth) // a.pool - first
    n_in = n_beams + 5
    torch.manual_seed(a.seed)
    nn = torch.nn
    policy = nn.Sequential(nn.Linear(n_in, a.hidden), nn.Tanh(), nn.Linear(a.hidden, a.hidden), nn.Tanh(), nn.Linear(a.hidden, 2), nn.Tanh())
    critic = nn.Sequential(nn.Linear(n_in, a.hidden), nn.Tanh(), nn.Linear(a.hidden, a.hidden), nn.Tanh(), nn.Linear(a.hidden, 1))
    fields = dict(pool=a.pool, max_range=10.0, beam_first=first, n_beams=n_beams, use_state=True, out_scale=(2.0, 0.6), out_offset=(2.5, 0.0))
    env = DeviceVecEnv(a.track, n_envs=a.envs, n_rays=a.rays, roster=["agent"], nets={0: net.from_torch(policy, **fields)},
                       action_repeat=a.repeat, max_episode_steps=a.episode, terminate_off_track=True, spawn_mode=1, seed=a.seed)
    env.set_value_net(0, critic)
    if a.device_update:
        env.train_begin(0)
    env.reset()
    dev = env.device
    policy, critic = policy.to(dev), critic.to(dev)
    scale, offset = torch.tensor(fields["out_scale"], device=dev), torch.tensor(fields["out_offset"], device=dev)
    std = torch.tensor([float(s) for s in a.std.split(",")], device=dev)
    opt = torch.optim.Adam(list(policy.parameters()) + list(critic.parameters()), lr=a.lr)
    T, roll = a.decisions, None
    for iteration in range(a.iterations):
        t0 = time.perf_counter()
        roll = env.collect(T, std=tuple(std.tolist()), clip=((0.0, 6.0), (-0.6, 0.6)), noise=True, values=True, gamma=a.gamma, lam=a.lam, out=roll)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if a.device_update:
            stats = env.ppo_update(roll, 0, epochs=a.epochs, minibatches=a.minibatches, lr=a.lr, clip=a.clip, value_coef=0.5, std=tuple(std.tolist()))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(json.dumps({"iteration": iteration, "update": "device", "reward_per_decision": float(roll.reward.mean()),
                              "return_mean": float(roll.returns.mean()), "value_mean": float(roll.value.mean()), "loss_pi": float(stats[-1, 1]),
                              "loss_v": float(stats[-1, 2]), "ends": int((roll.terminated | roll.truncated).sum()), "envs": a.envs, "decisions": T,
                              "collect_s": t1 - t0, "update_s": t2 - t1}), flush=True)
            continue
        x = roll.inputs.reshape(-1, n_in)
        z = roll.noise.reshape(-1, 2)
        proposed = roll.mean.reshape(-1, 2) + std * z                  # the action before the clip: what the behaviour policy drew
        old_logp = (-0.5 * z * z).sum(dim=1)                           # its log-density, up to the constant both policies share
        adv, ret = roll.advantage.reshape(-1), roll.returns.reshape(-1)
        n = x.shape[0]
        for _ in range(a.epochs):
            for idx in torch.randperm(n, device=dev).chunk(a.minibatches):
                mean = policy(x[idx]) * scale + offset
                logp = (-0.5 * ((proposed[idx] - mean) / std) ** 2).sum(dim=1)
                ratio = torch.exp(logp - old_logp[idx])
                ad = adv[idx]
                ad = (ad - ad.mean()) / (ad.std() + 1e-8)
                loss_pi = -torch.min(ratio * ad, ratio.clamp(1.0 - a.clip, 1.0 + a.clip) * ad).mean()
                loss_v = 0.5 * ((critic(x[idx]).squeeze(1) - ret[idx]) ** 2).mean()
                opt.zero_grad(set_to_none=True)
                (loss_pi + 0.5 * loss_v).backward()
                opt.step()
        env.set_net_params(0, flat(policy))
        env.set_value_params(0, flat(critic))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(json.dumps({"iteration": iteration, "update": "torch", "reward_per_decision": float(roll.reward.mean()), "return_mean": float(ret.mean()),
                          "value_mean": float(roll.value.mean()), "loss_pi": float(loss_pi), "loss_v": float(loss_v),
                          "ends": int((roll.terminated | roll.truncated).sum()), "envs": a.envs, "decisions": T,
                          "collect_s": t1 - t0, "update_s": t2 - t1}), flush=True)
    if a.save and a.device_update:
        net.NetSpec(env.env.net(0)[1], hidden_act="tanh", out_act="tanh", **fields).save(a.save)
    elif a.save:
        net.from_torch(policy.cpu(), **fields).save(a.save)
    env.close()


if __name__ == "__main__":
    main()
