"""A plain evolution-strategies loop on a network population: the usage example of ftgp_set_net_population, and the throughput tool's
companion (tools/net_throughput.py --rows population measures the launch; this shows the loop around it).

    python tools/evolve.py [--track circle] [--envs 1024] [--members 256] [--rays 1080] [--steps 400] [--generations 20]
                           [--sigma 0.05] [--lr 0.03] [--hidden 32] [--seed 0] [--save winner.npz]

One handle of --envs envs; slot 0 carries a population of --members members, env e running member e % members (so every member is
scored on envs / members random starts).  Per generation, all of it on the device but the fitness read-back:

    eps    = torch.randn([members / 2, count]), mirrored: (eps, -eps)
    params = theta + sigma * eps                          -> ftgp_set_net_population_device (no synchronisation)
    reset, rollout("net0", steps)                         ONE launch for the whole population
    fitness[m] = mean absolute completion (ftgp_get_progress column 3) of member m's envs
    theta += lr / (members * sigma) * sum_m rank_weight(fitness[m]) * eps[m]

and one JSON line: the generation, the best and the mean fitness, the wall time of the launch with its read-back.  Whether and how fast this learns
depends on the settings; nothing tests that.  Run it in a fresh process: torch is imported first (ft_grandprix_amd/vec.py).
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

from ft_grandprix_amd import capi, net  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--track", default="circle")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--generations", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="write the best member of the last generation as an .npz (net.load reads it)")
    a = ap.parse_args()
    if a.members < 2 or a.members % 2 or a.envs % a.members:
        raise SystemExit("--members: an even number that divides --envs")
    eighth = int(a.rays / 8.0)
    first = -(-eighth // a.pool)
    n_beams = (a.rays - eighth) // a.pool - first
    torch.manual_seed(a.seed)
    module = torch.nn.Sequential(torch.nn.Linear(n_beams + 5, a.hidden), torch.nn.Tanh(), torch.nn.Linear(a.hidden, 2), torch.nn.Tanh())
    spec = net.from_torch(module, pool=a.pool, max_range=10.0, beam_first=first, n_beams=n_beams, use_state=True, out_scale=(2.0, 0.6), out_offset=(2.5, 0.0))
    M, half, per = a.members, a.members // 2, a.envs // a.members
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev); gen.manual_seed(a.seed)
    theta = torch.from_numpy(spec.flat_params()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    lib = capi.load()
    with capi.Env(lib, load_track(a.track), n_envs=a.envs, n_rays=a.rays, spawn_mode=1, seed=a.seed) as g:
        g.set_net(0, spec.layers, **spec.input_fields())
        g.set_net_population(0, np.zeros((M, spec.param_count), dtype=np.float32))        # allocates; env e runs member e % M
        for generation in range(a.generations):
            eps = torch.randn((half, spec.param_count), generator=gen, device=dev)
            eps = torch.cat([eps, -eps])
            params = (theta[None, :] + a.sigma * eps).contiguous()
            g.set_net_population_device(0, params.data_ptr(), 0, stream)
            g.reset()
            t0 = time.perf_counter()
            g.rollout("net0", a.steps)
            done = g.progress()[:, 3].astype(np.float64).reshape(per, M)                  # env e = row e // M, member e % M
            wall = time.perf_counter() - t0                                               # (the read-back waits for the launch)
            fitness = done.mean(axis=0)
            rank = np.empty(M); rank[np.argsort(fitness)] = np.arange(M)
            weight = torch.from_numpy((rank / (M - 1) - 0.5).astype(np.float32)).to(dev)
            theta += a.lr / (M * a.sigma) * (weight[:, None] * eps).sum(dim=0)
            print(json.dumps({"generation": generation, "best": float(fitness.max()), "mean": float(fitness.mean()), "members": M, "envs": a.envs,
                              "steps": a.steps, "launch_s": wall, "member_steps_per_s": a.envs * a.steps / wall}), flush=True)
        if a.save:
            winner = spec.with_params(g.get_net_population(0, int(np.argmax(fitness))))
            winner.save(a.save)


if __name__ == "__main__":
    main()
