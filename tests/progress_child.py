"""Child process of tests/test_progress_search.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/progress_child.py <scenario> [json options]

`pool`: the pose pool of tests/progress_model.py on `ring` and `ring37` through one workgroup shape -- opt: n_envs, cars_per_block
(FTGP_CARS_PER_BLOCK, which ftgp_create reads: set before the handle exists; null = the plan's own choice), spawn_mode, via ("step": the
in-step search, "eval": progress_lane) -- against the model bit for bit and against an oracle twin on the same calls.
`two_tracks`: one ftgp_create_tracks handle holding `ring` and `ring37`, an oracle twin per env block.
`g5`: a G5 trace of the reference with the in-step search in its four-lane form (tests/helpers.replay_progress_trace, 8 envs).
The test asserts the workgroup shape of every handle from ftgp_create's FTGP_VERBOSE line.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library is loaded)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from tests import progress_model as pm  # noqa: E402
from tests.helpers import libs, replay_progress_trace  # noqa: E402

DEV = torch.device("cuda", 0)
R = 8


def workgroup_env(cars_per_block):
    os.environ["FTGP_VERBOSE"] = "1"
    if cars_per_block is None:
        os.environ.pop("FTGP_CARS_PER_BLOCK", None)
    else:
        os.environ["FTGP_CARS_PER_BLOCK"] = str(int(cars_per_block))


def check_offsets(env, spawn_mode):
    """The spawn index every car carries as its progress offset, read from an env-state record (include/ftgp.h: the int32 at byte
    136 + 8 of the car record), is the model's formula."""
    buf = torch.zeros((env.n_envs, env.env_state_bytes()), dtype=torch.uint8, device=DEV)
    env.save_envs_device(buf.data_ptr(), env.n_envs, 0, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    first = capi.env_state_layout(R, 1)["cars"] + 136 + 8
    got = np.ascontiguousarray(raw[:, first:first + 4]).view("<i4")[:, 0]
    want = np.array([pm.spawn_offset(spawn_mode, env.env_base + k, 0) for k in range(env.n_envs)])
    np.testing.assert_array_equal(got, want, err_msg="the offsets of the env-state records")
    np.testing.assert_array_equal(capi.unpack_env_state(raw, R, 1)["offset"][:, 0], want)
    return want


def after_reset(g, twins, model, what):
    """reset() runs progress_lane at the spawn pose, a centre-line point: completion 0, dist2 0.0 for every car."""
    model.completion[:] = 0
    model.update(g.pose()[:, 0:2])
    assert (model.completion == 0).all() and (model.dist2 == 0.0).all() and not model.off.any(), what
    np.testing.assert_array_equal(g.progress()[:, 1], model.completion, err_msg=f"{what}: completion")
    np.testing.assert_array_equal(g.progress()[:, 5], 0, err_msg=f"{what}: off_track")
    np.testing.assert_array_equal(g.centre_dist2(), model.dist2, err_msg=f"{what}: centre_dist2")
    for o, first, cars in twins:
        np.testing.assert_array_equal(g.progress()[first:first + cars], o.progress(), err_msg=f"{what}: progress() against the oracle")
        np.testing.assert_array_equal(g.race_steps()[first:first + cars], o.race_steps(), err_msg=f"{what}: race_steps()")


def pool(opt):
    lib, ora = libs()
    n, spawn_mode, via = int(opt["n_envs"]), int(opt.get("spawn_mode", 0)), opt.get("via", "step")
    workgroup_env(opt.get("cars_per_block"))
    poses = pm.pose_pool()
    seen = None
    for order in pm.ORDERS:
        track = pm.ring_track(order)
        kw = dict(n_envs=n, cars_per_env=1, n_rays=R, lap_target=pm.LAP_TARGET, spawn_mode=spawn_mode)
        with capi.Env(lib, track, **kw) as g, capi.Env(ora, track, **kw) as o:
            model = pm.Model(np.broadcast_to(track.path, (n, 100, 2)), check_offsets(g, spawn_mode))
            twins = [(o, 0, n)]
            after_reset(g, twins, model, f"{order}: after create")
            seen = pm.run_pool(g, model, poses, via, twins=twins, seen=seen, what=f"{order}, {n} envs")
            if via == "eval":
                g.reset(); o.reset()
                after_reset(g, twins, model, f"{order}: after reset()")
                mask = (np.arange(n) % 2).astype(np.uint8)                # ... and a masked one from wherever the pool left the cars
                seen = pm.run_pool(g, model, poses, via, twins=twins, seen=seen, passes=1, what=f"{order}, {n} envs, second run")
                before, d2 = g.progress(), g.centre_dist2()
                g.reset(mask); o.reset(mask)
                m = mask != 0
                assert (g.progress()[m, 1] == 0).all() and (g.centre_dist2()[m] == 0.0).all() and (g.progress()[m, 0] == 0).all()
                np.testing.assert_array_equal(g.progress()[~m], before[~m])
                np.testing.assert_array_equal(g.centre_dist2()[~m], d2[~m])
                np.testing.assert_array_equal(g.progress(), o.progress())
    print(f"pool ({via}, {n} envs): {seen}")
    pm.assert_seen(seen)
    print("pool ok")


def two_tracks(opt):
    lib, ora = libs()
    n, spawn_mode = int(opt.get("n_envs", 10)), int(opt.get("spawn_mode", 1))
    workgroup_env(opt.get("cars_per_block", 8))
    tracks = [pm.ring_track(order) for order in pm.ORDERS]
    counts = capi.split_envs(n, 2)
    firsts = [0, counts[0]]
    kw = dict(cars_per_env=1, n_rays=R, lap_target=pm.LAP_TARGET, spawn_mode=spawn_mode)
    g = capi.Env(lib, tracks, n_envs=n, **kw)
    twins = [(capi.Env(ora, t, n_envs=c, env_base=f, **kw), f, c) for t, c, f in zip(tracks, counts, firsts)]
    paths = np.stack([np.asarray(tracks[t].path, dtype=np.float64) for t in g.track_of_env])
    assert not np.array_equal(paths[0], paths[-1])
    model = pm.Model(paths, check_offsets(g, spawn_mode))
    after_reset(g, twins, model, "two tracks: after create")
    seen = pm.run_pool(g, model, pm.pose_pool(), "step", twins=twins, blocks=list(zip(firsts, counts)), what="two tracks")
    print(f"two tracks: {seen}")
    pm.assert_seen(seen)
    g.close()
    for o, _, _ in twins:
        o.close()
    print("two tracks ok")


def g5(opt):
    lib, _ = libs()
    workgroup_env(8)
    replay_progress_trace(lib, opt["trace"], n_envs=8)
    print("g5 ok")


SCENARIOS = {"pool": pool, "two_tracks": two_tracks, "g5": g5}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
