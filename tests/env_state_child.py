"""Child process of tests/test_env_state.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/env_state_child.py <scenario> [json options]

The criterion throughout is bit for bit: two states are equal when every read-back agrees byte by byte -- pose, progress, lap_times,
race_steps, ctrl, steps, lidar, centre_dist2, winners, episodes, dynamics.  What no read-back shows (the steering joint, the wheel
spins, fast.py's last steering angle) is covered by continuing: a state that differs there drives differently under nidc / fast.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: one HIP runtime per process)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402

DEV = torch.device("cuda", 0)
ERR_ARG, ERR_STATE = -1, -4
PER_CAR = ("pose", "progress", "lap_counts", "lap_times", "race_steps", "ctrl", "lidar", "centre_dist2", "winners", "dynamics")
PER_ENV = ("steps", "episodes")


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def rows_for(g, n_rows=None, fill=0):
    return torch.full((g.n_envs if n_rows is None else n_rows, g.env_state_bytes()), fill, dtype=torch.uint8, device=DEV)


def save(g, buf, mask=None):
    g.save_envs_device(buf.data_ptr(), buf.shape[0], 0 if mask is None else mask.data_ptr(), stream())


def load(g, buf, src=None):
    g.load_envs_device(buf.data_ptr(), buf.shape[0], 0 if src is None else src.data_ptr(), stream())


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def read_state(g):
    """Every read-back of a handle, per-car arrays as [n_envs, cars_per_env, ...]."""
    n, c = g.n_envs, g.cars_per_env
    counts, times = g.lap_times()
    s = dict(pose=g.pose(), progress=g.progress(), lap_counts=counts, lap_times=times, race_steps=g.race_steps(), ctrl=g.ctrl(),
             lidar=g.lidar(), centre_dist2=g.centre_dist2(), winners=g.winners(), dynamics=g.dynamics()[0])
    s = {k: np.ascontiguousarray(v).reshape(n, c, -1) for k, v in s.items()}
    s["steps"], s["episodes"] = g.steps().reshape(n, 1), g.episodes().reshape(n, 1)
    return s


def same_state(a, b, what, envs_a=None, envs_b=None):
    """Envs `envs_a` of state a equal envs `envs_b` of state b, byte by byte (None = all envs, in order)."""
    for key in PER_CAR + PER_ENV:
        x = a[key] if envs_a is None else a[key][list(envs_a)]
        y = b[key] if envs_b is None else b[key][list(envs_b)]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, key, x.shape, y.shape)
        if np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
            bad = np.flatnonzero([np.ascontiguousarray(x[e]).tobytes() != np.ascontiguousarray(y[e]).tobytes() for e in range(len(x))])
            raise AssertionError(f"{what}: {key} differs in envs (by position) {bad.tolist()}\n{x[bad[0]]}\n{y[bad[0]]}")


def differs(a, b, key="pose"):
    return np.ascontiguousarray(a[key]).tobytes() != np.ascontiguousarray(b[key]).tobytes()


def roster_of(cpe):
    return [("nidc", "fast")[c % 2] for c in range(cpe)]


def drive(g, policy, n):
    if g.cars_per_env > 1 and policy == "per_car":
        g.rollout("per_car", n)
    else:
        g.rollout(policy, n)


# ------------------------------------------------------------------------------------------------------------------ 1. layout
def layout(opt):
    lib = capi.load()
    track = load_track("circle")
    n, c, R = 19, 3, 90
    with capi.Env(lib, track, n_envs=n, cars_per_env=c, n_rays=R, spawn_mode=1, seed=5) as g:
        g.rollout("fast", 150)
        lay = capi.env_state_layout(R, c)
        assert g.env_state_bytes() == lay["bytes"], (g.env_state_bytes(), lay)
        buf = rows_for(g, fill=0xAB)
        save(g, buf)
        raw = buf.cpu().numpy()
        u = capi.unpack_env_state(raw, R, c)
        s = read_state(g)
        eq = np.testing.assert_array_equal
        eq(u["magic"], np.full(n, capi.ENV_STATE_MAGIC)); eq(u["version"], np.full(n, capi.ENV_STATE_VERSION))
        eq(u["n_rays"], np.full(n, R)); eq(u["cars_per_env"], np.full(n, c)); eq(u["lidar_mode"], np.zeros(n)); eq(u["reserved"], np.zeros(n))
        eq(u["fingerprint"], np.full(n, capi.track_fingerprint(track), dtype=np.uint64))
        eq(u["steps"], s["steps"][:, 0]); eq(u["steps"], np.full(n, 150)); eq(u["episodes"], np.zeros(n))
        pose = s["pose"]
        for name, col in (("x", 0), ("y", 1), ("qw", 3), ("qz", 6), ("vx", 7), ("vy", 8), ("wz", 12)):
            eq(u[name], pose[:, :, col], err_msg=name)
        eq(u["u_speed"], s["ctrl"][:, :, 0]); eq(u["u_steer"], s["ctrl"][:, :, 1])
        eq(u["dist2"], s["centre_dist2"][:, :, 0])
        prog = s["progress"]
        for name, col in (("laps", 0), ("completion", 1), ("finished", 4), ("off_track", 5), ("start", 6), ("good_start", 7), ("delta", 8)):
            eq(u[name], prog[:, :, col], err_msg=name)
        eq(u["n_times"], s["lap_counts"][:, :, 0]); eq(u["times"], s["lap_times"])
        eq(u["start"], s["race_steps"][:, :, 0])
        eq(u["ranges"], s["lidar"])
        eq(u["dyn"][:, :, :capi.DYN_DOUBLES], s["dynamics"])
        v = g.cfg.vehicle
        np.testing.assert_allclose(u["dyn"][:, :, capi.DYN_DOUBLES:].sum(axis=2), v.mass * v.gravity, rtol=1e-14)
        assert np.isfinite(u["qs"]).all() and np.isfinite(u["w"]).all() and (u["w"] != 0).any() and (u["last_steer"] != 0).any()
        # the bytes behind a scan row's last ray are zeros (90 rays: 360 of 368 bytes)
        rows = raw[:, lay["ranges"]:].reshape(n, c, lay["row_bytes"])
        assert lay["row_bytes"] == 368 and not rows[:, :, 4 * R:].any()
    print(f"layout ok: {lay['bytes']} bytes per env")


# ------------------------------------------------------------------------------------------------------------------ 2. restore
def restore_legs(a, b, leg, what, before_save=None, check_saved=None):
    """a and b are twins in the same state.  a saves, runs `leg`, loads, runs `leg` again; b runs `leg` once."""
    if before_save:
        for g in (a, b):
            before_save(g)
    buf = rows_for(a)
    save(a, buf)
    saved = read_state(a)
    if check_saved:
        check_saved(a)
    leg(a)
    first = read_state(a)
    leg(b)
    same_state(first, read_state(b), f"{what}: the twins' uninterrupted runs")
    assert differs(first, saved), f"{what}: the leg moved nothing"
    load(a, buf)
    same_state(read_state(a), saved, f"{what}: the state right after the load")
    leg(a)
    second = read_state(a)
    same_state(second, first, f"{what}: the leg after the load against the leg before it")
    return saved, first


def restore(opt):
    lib = capi.load()
    case = opt["case"]
    policy = opt.get("policy", "fast")
    N, M = 100, 120
    kw, track, start, leg, before_save, check_saved = dict(spawn_mode=1, seed=5), "small-circle", None, None, None, None
    if case == "one_car_1080":
        kw.update(n_envs=5, n_rays=1080)
    elif case == "eight_cars":
        kw.update(n_envs=3, cars_per_env=8, n_rays=64)
        track, policy = "circle", "per_car"
        t = load_track(track)
        along = (t.path[11] - t.path[10]) / np.linalg.norm(t.path[11] - t.path[10])

        def before_save(g):            # a pile-up: the cars of an env 0.1 apart, closer than two contact radii -- then one step
            pose = g.pose()
            for ci in range(g.n_cars):
                pose[ci, 0:2] = t.path[10] + 0.1 * (ci % 8) * along
            g.set_pose(pose)
            g.step(1)

        def check_saved(g):
            con = g.contacts()
            assert (con[:, 3] > 0).reshape(g.n_envs, 8).any(axis=1).all(), f"an env without car contacts at the saved state: {con}"
    elif case == "bubble_wrap":
        kw.update(n_envs=4, cars_per_env=3, n_rays=90, bubble_wrap=True)
        track, policy = "circle", "per_car"
    elif case == "tricycle":
        kw.update(n_envs=4, n_rays=64, dt=0.0075, vehicle=lib.tricycle_vehicle())
        ctrl = np.array([[0.6, 0.1], [0.8, -0.15], [0.5, 0.2], [0.7, 0.0]])

        def start(g):
            g.set_ctrl(ctrl)

        def leg(g, n=M):
            g.step(n)
    elif case == "fakelidar":
        kw.update(n_envs=5, n_rays=90, lidar_mode="fakelidar")
    else:
        raise SystemExit(f"unknown case {case}")
    if leg is None:
        def leg(g, n=M):
            drive(g, policy, n)
    with capi.Env(lib, load_track(track), **kw) as a, capi.Env(lib, load_track(track), **kw) as b:
        for g in (a, b):
            if g.cars_per_env > 1:
                g.set_car_policies(roster_of(g.cars_per_env))
            if start:
                start(g)
            leg(g, N)
        same_state(read_state(a), read_state(b), f"{case}: the twins after {N} steps")
        restore_legs(a, b, leg, case, before_save, check_saved)
    print(f"restore ok: {case} {policy}")


def teleport(g, envs, fracs, off=10):
    """The cars of `envs` (one car per env, spawn_mode 0: offset 10) visit the path points off + frac, one step each."""
    t = g.track
    for frac in fracs:
        pose = g.pose()
        for e in envs:
            pose[e, 0:2] = t.path[(off + frac) % 100]
        g.set_pose(pose)
        g.step(1)


def laps(opt):
    """Across a lap crossing (lap_target 5: n_times, times, start) or across a finish (lap_target 1: finished, finish_step, winners):
    envs 0 and 2 are walked round the track by set_pose (tests/helpers.py: laps_by_teleport), env 1 and 3 drive on."""
    lib = capi.load()
    target = int(opt["lap_target"])
    kw = dict(n_envs=4, n_rays=64, lap_target=target)
    moved = (0, 2)
    whole = (25, 50, 75, 99, 0)

    def leg(g):
        teleport(g, moved, (0, 25))            # the crossing, and on
        g.rollout("fast", 60)

    with capi.Env(lib, load_track("small-circle"), **kw) as a, capi.Env(lib, load_track("small-circle"), **kw) as b:
        for g in (a, b):
            g.rollout("fast", 40)
            if target > 1:
                teleport(g, moved[:1], whole)      # env 0 has a lap time already: the ring has an entry, start is not 0
            teleport(g, moved, whole[:4])          # up to the line
        saved, after = restore_legs(a, b, leg, f"lap_target {target}")
        crossed = after["lap_counts"][list(moved), 0, 0] - saved["lap_counts"][list(moved), 0, 0]
        assert (crossed == 1).all(), (saved["lap_counts"][:, 0, 0], after["lap_counts"][:, 0, 0])
        assert (after["race_steps"][list(moved), 0, 0] != saved["race_steps"][list(moved), 0, 0]).all()
        if target == 1:
            assert not saved["progress"][:, 0, 4].any() and after["progress"][list(moved), 0, 4].all(), after["progress"][:, 0, 4]
            assert after["winners"][list(moved), 0, 0].all() and not after["winners"][[1, 3], 0, 0].any()
        else:
            assert saved["lap_counts"][0, 0, 0] == 1 and after["lap_counts"][0, 0, 0] == 2 and not after["progress"][:, 0, 4].any()
    print(f"laps ok: lap_target {target}")


# ------------------------------------------------------------------------------------------------------------------ 3. masks
def masked(opt):
    lib = capi.load()
    n = 19
    kw = dict(n_envs=n, n_rays=64, spawn_mode=1, seed=5)
    track = load_track("small-circle")
    with capi.Env(lib, track, **kw) as a, capi.Env(lib, track, **kw) as b, capi.Env(lib, track, **kw) as c:
        for g in (a, b, c):
            g.rollout("fast", 100)
        # masked save: the rows of the other envs keep every byte
        picked = [2, 5, 18]
        mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
        mask[picked] = 1
        full, part = rows_for(a), rows_for(a, fill=0xAB)
        save(a, full)
        save(a, part, mask)
        full_h, part_h = full.cpu().numpy(), part.cpu().numpy()
        np.testing.assert_array_equal(part_h[picked], full_h[picked])
        rest = np.delete(part_h, picked, axis=0)
        assert (rest == 0xAB).all(), "a masked save wrote into the row of an env the mask leaves out"
        # selective load: a and b run on, a takes envs 1 and 7 back; every other env equals b, which never loaded
        back = [1, 7]
        others = [e for e in range(n) if e not in back]
        src = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        src[back] = torch.tensor(back, dtype=torch.int32, device=DEV)
        at_save = read_state(a)
        for g in (a, b):
            g.rollout("fast", 80)
        load(a, full, src)
        sa, sb = read_state(a), read_state(b)
        same_state(sa, sb, "envs with a negative src_row", others, others)
        same_state(sa, at_save, "envs taken back", back, back)
        assert differs(sb, at_save)
        for g in (a, b, c):
            g.rollout("fast", 60)
        sa, sb, sc = read_state(a), read_state(b), read_state(c)
        same_state(sa, sb, "envs with a negative src_row, 60 steps on", others, others)
        same_state(sa, sc, "envs taken back, 60 steps on", back, back)        # c: 100 + 60 steps, never loaded
        assert a.env_state_rejected() == 0
    print("masked ok")


# ------------------------------------------------------------------------------------------------------------------ 4. fork
def fork(opt):
    lib = capi.load()
    cpe = int(opt["cars"])
    n, K = 8, 150
    kw = dict(n_envs=n, cars_per_env=cpe, n_rays=64, spawn_mode=0, seed=5)
    track = load_track("circle" if cpe > 1 else "small-circle")
    policy = "per_car" if cpe > 1 else "fast"
    # spawn_mode 0 starts every env alike: the envs first drive on controls of their own
    ctrl = np.stack([np.linspace(0.8, 2.2, n * cpe), np.tile(np.linspace(-0.12, 0.12, n), cpe)], axis=1)
    for src in ([3] * n, [3, 3, 0, 7, 1, 1, 5, 2]):
        with capi.Env(lib, track, **kw) as a, capi.Env(lib, track, **kw) as b:
            for g in (a, b):
                if cpe > 1:
                    g.set_car_policies(roster_of(cpe))
                g.set_ctrl(ctrl)
                g.step(120)
            start = read_state(b)
            assert len({start["pose"][e].tobytes() for e in range(n)}) == n, "the envs do not differ before the fork"
            buf = rows_for(a)
            save(a, buf)
            load(a, buf, i32(src))
            same_state(read_state(a), start, f"right after the fork {src}", range(n), src)
            for g in (a, b):
                drive(g, policy, K)
            sb = read_state(b)
            same_state(read_state(a), sb, f"{K} steps after the fork {src}", range(n), src)
            assert differs(sb, start) and a.env_state_rejected() == 0
    print(f"fork ok: {cpe} cars")


# ------------------------------------------------------------------------------------------------------------------ 5. device step
def vec_env(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    case = opt["case"]
    n, calls = 12, 20
    kw = dict(n_envs=n, n_rays=64, cars_per_env=3, roster=["agent", "nidc", "agent"], scan_pool=4, scan_max_range=10.0, state=True,
              contacts=True, track_frame=True, lookahead=2, rivals=True, n_rivals=2, spawn_mode=1, seed=5,
              max_episode_steps=100000 if case == "plain" else 25)
    if case == "random_start":
        kw.update(random_start=True, start_lateral=0.5, start_yaw_jitter=0.2, shuffle_grid=True)
    if case == "dynamics":
        kw.update(randomize_dynamics={"friction": (0.3, 0.9), "mass": (4.0, 8.0)}, dynamics_seed=4)
    venv = DeviceVecEnv("circle", **kw)
    venv.reset()
    g = torch.Generator().manual_seed(3)
    acts = [(torch.rand((n, 2, 2), generator=g) * torch.tensor([2.0, 0.4]) + torch.tensor([0.5, -0.2])).to(DEV).contiguous() for _ in range(calls)]
    names = ("obs", "reward", "terminated", "truncated")

    def call(k):
        obs, reward, te, tr, info = venv.step(acts[k % calls])
        out = dict(obs=obs.clone(), reward=reward.clone(), terminated=te.clone(), truncated=tr.clone())
        out.update({key: v.clone() for key, v in info.items()})
        if venv.dynamics is not None:
            out["dynamics"] = venv.dynamics.clone()
        return out

    for k in range(17):
        last = call(k)
    snap = venv.save_state()
    assert snap.data.shape == (n, venv.bytes_per_env) and snap.data.dtype == torch.uint8 and snap.bytes_per_env == venv.env.env_state_bytes()
    episodes0 = venv.episode_index()
    first = [call(k) for k in range(calls)]
    table1 = venv.env.dynamics()[0]
    episodes1 = venv.episode_index()
    obs = venv.load_state(snap).clone()
    torch.cuda.synchronize()
    assert torch.equal(obs, last["obs"]), "obs right after load_state is not the obs of the call before the save"
    for key in ("state", "frame", "rival"):
        assert torch.equal(getattr(venv, key), last[key]), key
    np.testing.assert_array_equal(venv.episode_index(), episodes0)
    second = [call(k) for k in range(calls)]
    torch.cuda.synchronize()
    ended_calls = 0
    for k, (x, y) in enumerate(zip(first, second)):
        ended = x["terminated"] | x["truncated"]
        ended_calls += int(ended.any().item())
        for key in x:
            if key.startswith("final_"):       # only the rows of envs that ended in the call are written
                assert torch.equal(x[key][ended], y[key][ended]), (k, key)
            else:
                assert x[key].cpu().numpy().tobytes() == y[key].cpu().numpy().tobytes(), (k, key)
    np.testing.assert_array_equal(venv.episode_index(), episodes1)
    np.testing.assert_array_equal(venv.env.dynamics()[0], table1)
    if case == "plain":
        assert ended_calls == 0
    else:
        assert ended_calls >= 1, "no episode ended between the save and the load"
    if case == "random_start":
        assert (episodes1 > episodes0).all()
    if case == "dynamics":
        assert not torch.equal(first[0]["dynamics"], first[-1]["dynamics"]), "no redraw between the save and the load"
        np.testing.assert_array_equal(venv.dynamics.cpu().numpy().reshape(-1, 8), table1)
    assert venv.env.env_state_rejected() == 0
    # fork: every env continues from env 3
    src = torch.full((n,), 3, dtype=torch.int64, device=DEV)
    venv.fork(src)
    torch.cuda.synchronize()
    if case == "plain":
        s = read_state(venv.env)
        same_state(s, s, "fork(all from env 3)", range(n), [3] * n)
    venv.close()
    print(f"vec env ok: {case}, {ended_calls} calls with episode ends")


# ------------------------------------------------------------------------------------------------------------------ 6. cross-handle
def cross(opt):
    lib = capi.load()
    track = load_track("small-circle")
    kw = dict(n_envs=7, n_rays=64, spawn_mode=1, seed=5)
    with capi.Env(lib, track, **kw) as a, capi.Env(lib, track, **kw) as b:
        a.rollout("nidc", 150)
        buf = rows_for(a)
        save(a, buf)
        load(b, buf)
        same_state(read_state(b), read_state(a), "a fresh handle after the load")
        for g in (a, b):
            g.rollout("nidc", 100)
        same_state(read_state(b), read_state(a), "100 steps after the load")
        assert b.env_state_rejected() == 0
    # two tracks in one handle
    tracks = [load_track("small-circle"), load_track("circle")]
    counts = (3, 4)
    n = sum(counts)
    mkw = dict(n_envs=n, envs_per_track=counts, n_rays=64, spawn_mode=1, seed=5)
    with capi.Env(lib, tracks, **mkw) as a, capi.Env(lib, tracks, **mkw) as b:
        for g in (a, b):
            g.rollout("fast", 100)
        buf = rows_for(a)
        save(a, buf)
        u = capi.unpack_env_state(buf.cpu().numpy(), 64, 1)
        fps = np.array([capi.track_fingerprint(t) for t in tracks], dtype=np.uint64)
        np.testing.assert_array_equal(u["fingerprint"], fps[a.track_of_env])
        saved = read_state(a)
        a.rollout("fast", 80)
        load(a, buf)
        same_state(read_state(a), saved, "identity load on two tracks")
        a.rollout("fast", 80)
        b.rollout("fast", 80)
        same_state(read_state(a), read_state(b), "two tracks, after the load")
        assert a.env_state_rejected() == 0
        now = read_state(a)
        # rows of the other track: envs 0 and 6 stay as they are
        src = [-1] * n
        src[0], src[6] = 5, 1
        load(a, buf, i32(src))
        assert a.env_state_rejected() == 2, a.env_state_rejected()
        same_state(read_state(a), now, "rows of the other track")
        # an index past the rows
        src = [-1] * n
        src[4] = n
        load(a, buf, i32(src))
        assert a.env_state_rejected() == 3, a.env_state_rejected()
        small = buf[:2].clone()
        load(a, small, i32([0, 1, 2, -1, -1, -1, -1]))              # row 2 of 2 rows; rows 0 and 1 are taken
        assert a.env_state_rejected() == 4, a.env_state_rejected()
        same_state(read_state(a), saved, "rows 0 and 1 of a short buffer", [0, 1], [0, 1])
        same_state(read_state(a), now, "past the rows", range(2, n), range(2, n))
        now = read_state(a)
        # another version word
        other = buf.clone()
        other[2, 4] = 9
        other[5, 0] = 0
        src = [-1] * n
        src[2], src[5] = 2, 5
        load(a, other, i32(src))
        assert a.env_state_rejected() == 6, a.env_state_rejected()
        same_state(read_state(a), now, "another version, another magic")
        a.rollout("fast", 20)
    print("cross ok")


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def refused(call, code, text):
    try:
        call()
    except capi.FtgpError as x:
        assert x.code == code and text in str(x), x
    else:
        raise AssertionError(f"accepted: expected {code} {text}")


def errors(opt):
    lib = capi.load()
    track = load_track("small-circle")
    n = 6
    kw = dict(n_envs=n, n_rays=64, spawn_mode=1, seed=5)
    with capi.Env(lib, track, **kw) as a, capi.Env(lib, track, **kw) as b:
        for g in (a, b):
            g.rollout("fast", 60)
        bpe = a.env_state_bytes()
        good = rows_for(a)
        host = np.zeros((n, bpe), dtype=np.uint8)
        # The check knows an allocation's extent from the runtime, and torch carves small tensors out of larger allocations: 12 MB is an
        # allocation of its own, of `fit` whole records.
        big = torch.zeros(12 << 20, dtype=torch.uint8, device=DEV)
        fit = (12 << 20) // bpe
        few = rows_for(a, n - 1)
        host_src = np.zeros(n, dtype=np.int32)
        for entry, fn in (("ftgp_save_envs_device", a.save_envs_device), ("ftgp_load_envs_device", a.load_envs_device)):
            refused(lambda: fn(host.ctypes.data, n, 0, stream()), ERR_ARG, entry)
            refused(lambda: fn(big.data_ptr(), fit + 1, 0, stream()), ERR_ARG, entry)
            refused(lambda: fn(few.data_ptr(), n - 1, 0, stream()), ERR_ARG, entry)
            refused(lambda: fn(good.data_ptr(), 0, 0, stream()), ERR_ARG, entry)
            refused(lambda: fn(good.data_ptr() + 8, n - 1, 0, stream()), ERR_ARG, entry)
            refused(lambda: fn(good.data_ptr(), n, host_src.ctypes.data, stream()), ERR_ARG, entry)
        obs = torch.zeros((n, 1, 64), dtype=torch.float32, device=DEV)
        refused(lambda: a.obs_device(obs.data_ptr(), stream()), ERR_STATE, "ftgp_obs_device")
        torch.cuda.synchronize()
        assert not good.any().item() and not big.any().item() and a.env_state_rejected() == 0
        for g in (a, b):
            g.rollout("fast", 1)
        same_state(read_state(a), read_state(b), "a step after the refusals")
        a.save_envs_device(big.data_ptr(), fit, 0, stream())           # as many rows as the allocation holds: taken
        torch.cuda.synchronize()
        assert big[:n * bpe].any().item() and not big[n * bpe:].any().item()
        a.device_io_config(None, 0, 1, True)
        a.obs_device(obs.data_ptr(), stream())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(obs.cpu().numpy().reshape(n, 64), a.lidar())
    print("errors ok")


# ------------------------------------------------------------------------------------------------------------------ 8. nothing else moved
def neutral(opt):
    lib = capi.load()
    track = load_track("small-circle")
    kw = dict(n_envs=19, n_rays=64, spawn_mode=1, seed=5)
    with capi.Env(lib, track, **kw) as a, capi.Env(lib, track, **kw) as b:
        name = b.kernel_name()
        assert name.startswith("ftgp_step_kernel<") and a.kernel_name() == name, (name, a.kernel_name())
        buf = rows_for(a)
        for launch in range(3):
            save(a, buf)
            load(a, buf)
            for g in (a, b):
                g.rollout("fast", 100)
            same_state(read_state(a), read_state(b), f"launch {launch}")
            np.testing.assert_array_equal(a.metrics_local(), b.metrics_local())
            assert a.kernel_name() == b.kernel_name() == name, (a.kernel_name(), b.kernel_name(), name)
        assert a.dynamics()[1] == 0 and a.env_state_rejected() == 0
    print(f"neutral ok: {name}")


SCENARIOS = {"layout": layout, "restore": restore, "laps": laps, "masked": masked, "fork": fork, "vec_env": vec_env, "cross": cross,
             "errors": errors, "neutral": neutral}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
