"""What a network driver costs a step: rollout("net0") against rollout("fast") and rollout("lobotomy"), and against the device step
with one agent whose network torch evaluates.

    python tools/net_throughput.py [--envs 4096] [--rays 1080] [--steps 500] [--launches 5] [--track track] [--calls 500]
                                   [--decisions 100] [--rows rollout,agent,collect,roster,collect2,population,sequential]
                                   [--members 1,64,4096]

rollout rows: one launch of --steps steps per measurement, --launches of them after one warm-up launch; env-steps/s from the wall clock
around the launch and its synchronisation, and the step kernel's own time from ftgp_last_kernel_ms.  The network is a random
85 -> 64 -> 64 -> 2 tanh MLP on beams 14 .. 93 of pool 10 and the five state inputs (at another --rays: the beams of the scan window).
The "rollout net0 frame" and "collect ... frame inputs" rows run an 85 + 4 + 2 * 8 -> 64 -> 64 -> 2 network: the same inputs and the
track-frame row with eight look-ahead points behind them (ftgp_set_net_frame) -- what the frame inputs cost beside the same network
without them.
roster rows (--rows roster): --envs envs of FOUR cars, a roster of four network slots, rollout("per_car"): the 85 -> 64 -> 64 -> 2 network
in every slot, and the same network with the rival row of three mate slots behind its inputs (85 + 4 + 8 * 3 -> ..., ftgp_set_net_rivals)
-- what the rival inputs cost, and the MULTI NET step kernels' timing.  us per step is the launch's; per decision it is that over the
four cars.  collect2 rows (--rows collect2): collect with two agents and two bundled cars per env, without and with the rival inputs.
population rows (--rows population): the rollout row's network as a population (ftgp_set_net_population) of --members members on
--envs envs, env e running member e % M, every member a perturbation of the network drawn by torch on the device and handed over by
ftgp_set_net_population_device: one launch of --steps steps runs them all.  member_steps_per_s = envs x steps over the wall clock.
sequential row (--rows sequential): the way without a population, for the middle --members entry M: ONE handle of envs / M envs, and
per member an ftgp_set_net_device and a launch of --steps steps, M launches; member_steps_per_s = envs x steps over the wall clock
of the M launches.  It uses no population entry, so the same file runs on a tree from before them.
agent row: DeviceVecEnv(roster=["agent"], scan_pool, scan_max_range, state=True), the same network as an nn.Sequential evaluated by
torch before every call, --calls calls of one step; per-call time from HIP events on torch's stream.
collect row: the same env with the network in slot 0, DeviceVecEnv.collect (ftgp_collect_device) of --decisions decisions a call with
noise drawn by one torch.randn, next_inputs on; --launches calls after one warm-up call; per-decision time from HIP events around the
calls, env-steps/s from the wall clock -- the row to hold against the agent row of the same run.  One JSON line per row.  Run it in
a fresh process: torch is imported first (ft_grandprix_amd/vec.py).  Under `rocprofv3 --kernel-trace --stats -- python
tools/net_throughput.py --rows rollout` (or `--rows collect`) the per-kernel times come out of the stats file.
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


def make_module(n_in):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 2), torch.nn.Tanh())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--decisions", type=int, default=100)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--track", default="track")
    ap.add_argument("--rows", default="rollout,agent")
    ap.add_argument("--members", default="1,64,4096")
    a = ap.parse_args()
    eighth = int(a.rays / 8.0)
    first = -(-eighth // a.pool)
    n_beams = (a.rays - eighth) // a.pool - first
    fields = dict(pool=a.pool, max_range=10.0, beam_first=first, n_beams=n_beams, use_state=True, out_scale=(2.0, 0.6), out_offset=(2.5, 0.0))
    module = make_module(n_beams + 5)
    spec = net.from_torch(module, **fields)
    spec_frame = net.from_torch(make_module(n_beams + 5 + 4 + 2 * 8), lookahead=8, lookahead_stride=1, **fields)
    spec_rivals = net.from_torch(make_module(n_beams + 5 + 4 + 8 * 3), n_rivals=3, **fields)
    track = load_track(a.track)
    rows = a.rows.split(",")
    if "rollout" in rows:
        lib = capi.load()
        for policy, what in (("lobotomy", None), ("fast", None), ("net0", spec), ("net0", spec_frame)):
            with capi.Env(lib, track, n_envs=a.envs, n_rays=a.rays, spawn_mode=1, seed=7) as g:
                if what is not None:
                    g.set_net(0, what.layers, **what.input_fields())
                g.rollout(policy, a.steps)
                g.steps()
                wall, kern = [], []
                for _ in range(a.launches):
                    t0 = time.perf_counter()
                    g.rollout(policy, a.steps)
                    kern.append(g.last_kernel_ms())
                    wall.append(time.perf_counter() - t0)
                print(json.dumps({"row": f"rollout {policy}" + (" frame" if what is spec_frame else ""), "envs": a.envs, "rays": a.rays, "steps": a.steps, "kernel": g.kernel_name(),
                                  "env_steps_per_s": a.envs * a.steps / float(np.median(wall)), "kernel_ms_median": float(np.median(kern)),
                                  "kernel_us_per_step": 1e3 * float(np.median(kern)) / a.steps, "off_track": int(g.progress()[:, 5].sum())}), flush=True)
    members = [int(m) for m in a.members.split(",")]

    def perturbed(n):
        gen = torch.Generator(device="cuda"); gen.manual_seed(n)
        theta = torch.from_numpy(spec.flat_params()).to("cuda")
        return (theta[None, :] + 0.05 * torch.randn((n, theta.numel()), generator=gen, device="cuda")).contiguous()
    if "population" in rows:
        lib = capi.load()
        stream = torch.cuda.current_stream().cuda_stream
        for M in members:
            with capi.Env(lib, track, n_envs=a.envs, n_rays=a.rays, spawn_mode=1, seed=7) as g:
                g.set_net(0, spec.layers, **spec.input_fields())
                params = perturbed(M)
                # what one car reads of its member per step: every layer's n_in rows and its bias, each padded to 64 floats (the library's layout)
                w = spec.widths
                row_bytes = sum((w[l] + 1) * 4 * 64 * -(-w[l + 1] // 64) for l in range(len(w) - 1))
                g.set_net_population(0, np.zeros((M, spec.param_count), dtype=np.float32))       # allocates; the members come from the device
                g.set_net_population_device(0, params.data_ptr(), 0, stream)
                g.rollout("net0", a.steps)
                g.steps()
                wall, kern = [], []
                for _ in range(a.launches):
                    t0 = time.perf_counter()
                    g.set_net_population_device(0, params.data_ptr(), 0, stream)                # a generation's hand-over is part of its cost
                    g.rollout("net0", a.steps)
                    kern.append(g.last_kernel_ms())
                    wall.append(time.perf_counter() - t0)
                us = 1e3 * float(np.median(kern)) / a.steps
                print(json.dumps({"row": f"population of {M}", "members": M, "envs": a.envs, "rays": a.rays, "steps": a.steps, "kernel": g.kernel_name(),
                                  "member_steps_per_s": a.envs * a.steps / float(np.median(wall)), "kernel_ms_median": float(np.median(kern)),
                                  "kernel_us_per_step": us, "weights_MB_per_step_if_unshared": 1e-6 * row_bytes * a.envs,
                                  "off_track": int(g.progress()[:, 5].sum())}), flush=True)
    if "sequential" in rows:
        lib = capi.load()
        stream = torch.cuda.current_stream().cuda_stream
        M = members[len(members) // 2]
        with capi.Env(lib, track, n_envs=a.envs // M, n_rays=a.rays, spawn_mode=1, seed=7) as g:
            g.set_net(0, spec.layers, **spec.input_fields())
            params = perturbed(M)
            g.rollout("net0", a.steps)
            g.steps()
            wall, kern = [], []
            for _ in range(a.launches):
                t0 = time.perf_counter()
                k = 0.0
                for m in range(M):
                    g.set_net_device(0, params[m].data_ptr(), stream)
                    g.rollout("net0", a.steps)
                    k += g.last_kernel_ms()
                wall.append(time.perf_counter() - t0)
                kern.append(k)
            print(json.dumps({"row": f"sequential: {M} launches of {a.envs // M} envs", "members": M, "envs": a.envs // M, "rays": a.rays, "steps": a.steps,
                              "kernel": g.kernel_name(), "member_steps_per_s": (a.envs // M) * M * a.steps / float(np.median(wall)),
                              "kernel_ms_median_all_launches": float(np.median(kern)), "kernel_us_per_step_one_launch": 1e3 * float(np.median(kern)) / (M * a.steps)}), flush=True)
    if "roster" in rows:
        lib = capi.load()
        for what, label in ((spec, "roster of four net slots"), (spec_rivals, "roster of four net slots, rival inputs")):
            with capi.Env(lib, track, n_envs=a.envs, cars_per_env=4, n_rays=a.rays, spawn_mode=1, seed=7) as g:
                for s in range(4):
                    g.set_net(s, what.layers, **what.input_fields())
                g.set_car_policies(["net0", "net1", "net2", "net3"])
                g.rollout("per_car", a.steps)
                g.steps()
                wall, kern = [], []
                for _ in range(a.launches):
                    t0 = time.perf_counter()
                    g.rollout("per_car", a.steps)
                    kern.append(g.last_kernel_ms())
                    wall.append(time.perf_counter() - t0)
                us = 1e3 * float(np.median(kern)) / a.steps
                print(json.dumps({"row": label, "n_in": what.n_in, "envs": a.envs, "cars_per_env": 4, "rays": a.rays, "steps": a.steps, "kernel": g.kernel_name(),
                                  "env_steps_per_s": a.envs * a.steps / float(np.median(wall)), "kernel_ms_median": float(np.median(kern)),
                                  "kernel_us_per_step": us, "kernel_ns_per_decision": 1e3 * us / (4 * a.envs), "off_track": int(g.progress()[:, 5].sum())}), flush=True)
    if "agent" in rows:
        from ft_grandprix_amd.vec import DeviceVecEnv
        venv = DeviceVecEnv(track, n_envs=a.envs, n_rays=a.rays, roster=["agent"], scan_pool=a.pool, scan_max_range=10.0, state=True, spawn_mode=1, seed=7)
        dev = venv.device
        policy = module.to(dev)
        scale, offset = torch.tensor(fields["out_scale"], device=dev), torch.tensor(fields["out_offset"], device=dev)
        obs, state = venv.reset(), venv.state

        @torch.no_grad()
        def act():
            x = torch.cat([obs[:, 0, first:first + n_beams], state[:, 0, :5]], dim=1)
            return (policy(x) * scale + offset)[:, None, :].contiguous()
        for _ in range(20):
            venv.step(act())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.calls):
            venv.step(act())
        e1.record()
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        print(json.dumps({"row": "device step, torch evaluates the network", "envs": a.envs, "rays": a.rays, "calls": a.calls,
                          "env_steps_per_s": a.envs * a.calls / wall, "us_per_call_events": 1e3 * e0.elapsed_time(e1) / a.calls}), flush=True)
        venv.close()
    collect_rows = ((spec, "collect, network on the device", ["agent"]), (spec_frame, "collect, network on the device, frame inputs", ["agent"])) if "collect" in rows else ()
    if "collect2" in rows:
        two = ["agent", "fast", "agent", "fast"]
        collect_rows += ((spec, "collect, two agents of four cars", two), (spec_rivals, "collect, two agents of four cars, rival inputs", two))
    for the_spec, label, roster in collect_rows:
        from ft_grandprix_amd.vec import DeviceVecEnv
        venv = DeviceVecEnv(track, n_envs=a.envs, n_rays=a.rays, cars_per_env=len(roster), roster=roster, scan_pool=a.pool, scan_max_range=10.0, state=True, spawn_mode=1,
                            seed=7, nets={0: the_spec})
        dev = venv.device
        venv.reset()
        kw = dict(std=(0.3, 0.1), clip=((0.0, 5.0), (-0.6, 0.6)), noise=True, next_inputs=True)
        roll = venv.collect(a.decisions, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.launches):
            roll = venv.collect(a.decisions, out=roll, **kw)
        e1.record()
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        n = a.launches * a.decisions
        print(json.dumps({"row": label, "n_in": the_spec.n_in, "envs": a.envs, "agents_per_env": roster.count("agent"), "rays": a.rays, "calls": a.launches, "decisions_per_call": a.decisions,
                          "env_steps_per_s": a.envs * n / wall, "us_per_decision_events": 1e3 * e0.elapsed_time(e1) / n,
                          "us_per_decision_wall": 1e6 * wall / n, "ends": int((roll.terminated | roll.truncated).sum())}), flush=True)
        venv.close()


if __name__ == "__main__":
    main()
