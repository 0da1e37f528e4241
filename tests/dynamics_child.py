"""Child process of tests/test_dynamics.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/dynamics_child.py <scenario> [json options]

The criterion of every twin scenario: car a of a handle with the dynamics table on equals, bit for bit, car a of a CPU-oracle handle
that has no table and whose vehicle carries the row's eight values (the oracle takes a vehicle and equals the GPU bit for bit).
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
from tests import helpers  # noqa: E402

LO, HI = helpers.DYN_LO, helpers.DYN_HI             # (tests/test_free_step.py draws its rows between the same)
LOOP = dict(n_rays=64, spawn_mode=1, seed=5)          # the closed loop of scenario 1
ERR_ARG, ERR_STATE = -1, -4


def make_rows(base, n, seed):
    return base * np.random.default_rng(seed).uniform(LO, HI, (n, 8))


def vehicle_with(base_vehicle, row):
    """A copy of the vehicle with the eight dynamics fields replaced by `row`."""
    v = capi.FtgpVehicle.from_buffer_copy(base_vehicle)
    for f, x in zip(capi.DYN_FIELDS, row):
        setattr(v, f, float(x))
    return v


class EnvView:
    """Env `e` of a handle as a one-env handle would show it: what helpers.assert_same_state reads, from one set of read-backs."""

    def __init__(self, snap, e, cpe):
        self.s, self.cars, self.e = snap, slice(e * cpe, (e + 1) * cpe), e

    def progress(self): return self.s["progress"][self.cars]
    def steps(self): return self.s["steps"][self.e:self.e + 1]
    def lap_times(self): return self.s["lap_times"][0][self.cars], self.s["lap_times"][1][self.cars]
    def lidar(self): return self.s["lidar"][self.cars]
    def pose(self): return self.s["pose"][self.cars]
    def ctrl(self): return self.s["ctrl"][self.cars]
    def snapshot(self): return self.s["snapshot"][self.cars]


def read_back(g):
    return dict(progress=g.progress(), steps=g.steps(), lap_times=g.lap_times(), lidar=g.lidar(), pose=g.pose(), ctrl=g.ctrl(),
                snapshot=g.snapshot())


def assert_envs_match(g, twins, cpe, what):
    snap = read_back(g)
    for e, o in enumerate(twins):
        try:
            helpers.assert_same_state(EnvView(snap, e, cpe), o)
            np.testing.assert_array_equal(snap["ctrl"][e * cpe:(e + 1) * cpe], o.ctrl())
            np.testing.assert_array_equal(snap["pose"][e * cpe:(e + 1) * cpe], o.pose())
        except AssertionError as x:
            raise AssertionError(f"{what}, env {e}\n{x}") from None


def is_dynamics_kernel(name):
    return name.startswith("ftgp_step_kernel<") and name.count(",") == 4 and name.endswith(", true>")


def closed_loop(opt):
    lib, ora = helpers.libs()
    track = load_track("small-circle")
    n = 19
    with capi.Env(lib, track, n_envs=n, **LOOP) as g, capi.Env(lib, track, n_envs=n, **LOOP) as plain:
        rows = make_rows(g.base_dynamics(), n, 11)
        g.set_dynamics(rows.reshape(n, 1, 8))
        twins = [capi.Env(ora, track, n_envs=1, env_base=e, vehicle=vehicle_with(g.cfg.vehicle, rows[e]), **LOOP) for e in range(n)]
        for launch in range(3):
            g.rollout("fast", 100)
            for o in twins:
                o.rollout("fast", 100)
            assert_envs_match(g, twins, 1, f"launch {launch}")
        got, rejected = g.dynamics()
        np.testing.assert_array_equal(got, rows)
        assert rejected == 0, rejected
        name = g.kernel_name()
        assert is_dynamics_kernel(name), name
        plain.rollout("fast", 300)
        a, b = g.pose(), plain.pose()
        assert np.isfinite(a).all() and np.isfinite(b).all()
        differs = (a != b).any(axis=1)
        assert differs.all(), f"envs whose pose equals the default vehicle's: {np.flatnonzero(~differs)}"
        for o in twins:
            o.close()
    print(f"closed loop ok: kernel {name}")


def multi_car(opt):
    lib, ora = helpers.libs()
    cpe, bubble, n = int(opt["cars_per_env"]), bool(opt.get("bubble_wrap", False)), 5
    track = load_track("circle")
    roster = [("nidc", "fast")[c % 2] for c in range(cpe)]
    kw = dict(cars_per_env=cpe, n_rays=90, spawn_mode=1, seed=5, bubble_wrap=bubble)
    with capi.Env(lib, track, n_envs=n, **kw) as g:
        rows = make_rows(g.base_dynamics(), n, 11)
        g.set_dynamics(np.repeat(rows[:, None, :], cpe, axis=1))
        g.set_car_policies(roster)
        twins = [capi.Env(ora, track, n_envs=1, env_base=e, vehicle=vehicle_with(g.cfg.vehicle, rows[e]), **kw) for e in range(n)]
        g.rollout("per_car", 300)
        for o in twins:
            o.set_car_policies(roster)
            o.rollout("per_car", 300)
        assert_envs_match(g, twins, cpe, f"{cpe} cars per env")
        assert is_dynamics_kernel(g.kernel_name()), g.kernel_name()
        for o in twins:
            o.close()
    print(f"multi car ok: {cpe} cars per env, bubble_wrap {bubble}")


def distinct_rows(opt):
    lib, ora = helpers.libs()
    cars = int(opt["cars"])
    track = helpers.open_field()
    kw = dict(n_envs=1, cars_per_env=cars, n_rays=8)
    ctrl = np.tile([1.5, 0.15], (cars, 1))
    with capi.Env(lib, track, **kw) as g:
        rows = make_rows(g.base_dynamics(), cars, 7)
        g.set_dynamics(rows.reshape(1, cars, 8))
        twins = [capi.Env(ora, track, vehicle=vehicle_with(g.cfg.vehicle, rows[a]), **kw) for a in range(cars)]
        for env in [g] + twins:
            env.set_ctrl(ctrl)
        closest = np.inf
        for k in range(30):
            g.step(10)
            pose = g.pose()
            xy = pose[:, 0:2]
            d = np.hypot(*(xy[:, None, :] - xy[None, :, :]).transpose(2, 0, 1))
            d[np.diag_indices(cars)] = np.inf
            assert d.min() >= 0.5, f"cars {np.unravel_index(d.argmin(), d.shape)} are {d.min()} apart after {10 * (k + 1)} steps: a contact could couple them"
            closest = min(closest, d.min())
            for a, o in enumerate(twins):
                o.step(10)
                np.testing.assert_array_equal(pose[a], o.pose()[a], err_msg=f"car {a} after {10 * (k + 1)} steps")
        assert is_dynamics_kernel(g.kernel_name()), g.kernel_name()
        for o in twins:
            o.close()
    print(f"distinct rows ok: {cars} cars, smallest distance {closest:.3f}")


def neutral(opt):
    lib = capi.load()
    track = load_track("small-circle")
    n = 19
    with capi.Env(lib, track, n_envs=n, **LOOP) as a, capi.Env(lib, track, n_envs=n, **LOOP) as b:
        base = a.base_dynamics()
        a.set_dynamics(np.tile(base, (n, 1, 1)))
        old_name = b.kernel_name()
        for launch in range(2):
            a.rollout("fast", 100)
            b.rollout("fast", 100)
            helpers.same(a, b, f"neutral rows, launch {launch}")
            np.testing.assert_array_equal(a.pose(), b.pose())
        assert is_dynamics_kernel(a.kernel_name()) and not is_dynamics_kernel(b.kernel_name()), (a.kernel_name(), b.kernel_name())
        a.set_dynamics(None)
        assert a.kernel_name() == b.kernel_name() == old_name, (a.kernel_name(), old_name)
        got, rejected = a.dynamics()
        np.testing.assert_array_equal(got, np.tile(base, (n, 1)))
        assert rejected == 0
        a.rollout("fast", 50)
        b.rollout("fast", 50)
        helpers.same(a, b, "after the table was turned off")
    print("neutral ok")


def device_setter(opt):
    lib, ora = helpers.libs()
    track = load_track("small-circle")
    n = 19
    dev = torch.device("cuda", 0)
    masked = [2, 5, 18]
    mask = np.zeros(n, dtype=np.uint8)
    mask[masked] = 1
    with capi.Env(lib, track, n_envs=n, **LOOP) as h, capi.Env(lib, track, n_envs=n, **LOOP) as d:
        base = d.base_dynamics()
        rows = make_rows(base, n, 11)
        h.set_dynamics(rows.reshape(n, 1, 8), mask)
        rows_t, mask_t = torch.from_numpy(rows).to(dev), torch.from_numpy(mask).to(dev)
        d.set_dynamics_device(rows_t.data_ptr(), mask_t.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        want, _ = h.dynamics()
        got, rejected = d.dynamics()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got[masked], rows[masked])
        np.testing.assert_array_equal(np.delete(got, masked, axis=0), np.tile(base, (n - 3, 1)))
        assert rejected == 0 and is_dynamics_kernel(d.kernel_name())
        # invalid rows: the car keeps its old row, the counter says how many
        rows2 = make_rows(base, n, 12)
        rows2[2, 0] = -1.0
        rows2[5, 2] = np.nan
        rows2_t = torch.from_numpy(rows2).to(dev)
        d.set_dynamics_device(rows2_t.data_ptr(), mask_t.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        got2, rejected = d.dynamics()
        want2 = want.copy()
        want2[18] = rows2[18]
        np.testing.assert_array_equal(got2, want2)
        assert rejected == 2, rejected
        # a host pointer: refused before anything is enqueued
        try:
            d.set_dynamics_device(rows.ctypes.data)
        except capi.FtgpError as x:
            assert x.code == ERR_ARG, x
        else:
            raise AssertionError("a host pointer was accepted")
        np.testing.assert_array_equal(d.dynamics()[0], want2)
        # ordering: rows computed on a side stream, the setter and a device step right behind them, no host synchronisation
        d.device_io_config(None, 0, 1, True)
        factors = np.random.default_rng(13).uniform(LO, HI, (n, 8))
        side = torch.cuda.Stream(dev)
        obs = torch.zeros((n, 1, LOOP["n_rays"]), dtype=torch.float32, device=dev)
        reward = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        term, trunc = torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
        act = torch.tensor([1.5, 0.15], dtype=torch.float32, device=dev).repeat(n, 1, 1).contiguous()
        base_t, factors_t = torch.from_numpy(base).to(dev), torch.from_numpy(factors).to(dev)
        torch.cuda.synchronize()
        calls = 20
        with torch.cuda.stream(side):
            rows3_t = (base_t * factors_t).contiguous()
            d.set_dynamics_device(rows3_t.data_ptr(), 0, side.cuda_stream)
            for _ in range(calls):
                d.step_device(act.data_ptr(), obs.data_ptr(), reward.data_ptr(), term.data_ptr(), trunc.data_ptr(), stream=side.cuda_stream)
        torch.cuda.synchronize()
        rows3 = base * factors
        np.testing.assert_array_equal(d.dynamics()[0], rows3)
        pose = d.pose()
        ctrl = np.array([[1.5, float(np.float32(0.15))]])
        for e in range(n):
            with capi.Env(ora, track, n_envs=1, env_base=e, vehicle=vehicle_with(d.cfg.vehicle, rows3[e]), **LOOP) as o:
                o.set_ctrl(ctrl)
                o.step(calls)
                np.testing.assert_array_equal(pose[e], o.pose()[0], err_msg=f"env {e} after the side-stream calls")
        assert not term.any().item() and not trunc.any().item()
    print("device setter ok")


def multitrack(opt):
    lib, ora = helpers.libs()
    tracks = [load_track("small-circle"), load_track("circle")]
    counts = (3, 4)
    n = sum(counts)
    with capi.Env(lib, tracks, n_envs=n, envs_per_track=counts, **LOOP) as g:
        rows = make_rows(g.base_dynamics(), n, 11)
        g.set_dynamics(rows.reshape(n, 1, 8))
        twins = [capi.Env(ora, tracks[g.track_of_env[e]], n_envs=1, env_base=e, vehicle=vehicle_with(g.cfg.vehicle, rows[e]), **LOOP)
                 for e in range(n)]
        for launch in range(2):
            g.rollout("fast", 100)
            for o in twins:
                o.rollout("fast", 100)
            assert_envs_match(g, twins, 1, f"multi-track, launch {launch}")
        name = g.kernel_name()
        assert is_dynamics_kernel(name) and name.endswith("true, true>"), name
        for o in twins:
            o.close()
    print("multitrack ok")


def tricycle(opt):
    lib, ora = helpers.libs()
    track = load_track("small-circle")
    n = 4
    kw = dict(dt=0.0075, **LOOP)
    veh = lib.tricycle_vehicle()
    ctrl = np.array([[0.6, 0.1], [0.8, -0.15], [0.5, 0.2], [0.7, 0.0]])
    with capi.Env(lib, track, n_envs=n, vehicle=veh, **kw) as g:
        base = g.base_dynamics()
        factors = np.random.default_rng(11).uniform(LO, HI, (n, 8))
        factors[:, 4:] = 1.0                          # a tricycle reads entries 0-3 only
        rows = base * factors
        g.set_dynamics(rows.reshape(n, 1, 8))
        twins = [capi.Env(ora, track, n_envs=1, env_base=e, vehicle=vehicle_with(veh, rows[e]), **kw) for e in range(n)]
        g.set_ctrl(ctrl)
        for e, o in enumerate(twins):
            o.set_ctrl(ctrl[e:e + 1])
        for launch in range(2):
            g.step(100)
            for o in twins:
                o.step(100)
            assert_envs_match(g, twins, 1, f"tricycle, launch {launch}")
        assert is_dynamics_kernel(g.kernel_name()), g.kernel_name()
        with capi.Env(lib, track, n_envs=n, vehicle=veh, **kw) as plain:
            plain.set_ctrl(ctrl)
            plain.step(200)
            assert ((g.pose() != plain.pose()).any(axis=1)).all()
        for o in twins:
            o.close()
    print("tricycle ok")


def errors(opt):
    lib = capi.load()
    track = load_track("small-circle")
    dev = torch.device("cuda", 0)
    with capi.Env(lib, track, n_envs=4, n_rays=36, lidar_mode="fakelidar") as f:
        rows = np.tile(f.base_dynamics(), (4, 1, 1))
        rows_t = torch.from_numpy(rows).to(dev)
        for call in (lambda: f.set_dynamics(rows), lambda: f.set_dynamics_device(rows_t.data_ptr())):
            try:
                call()
            except capi.FtgpError as x:
                assert x.code == ERR_STATE, x
            else:
                raise AssertionError("a FAKELIDAR handle took a dynamics table")
        assert not is_dynamics_kernel(f.kernel_name())
    with capi.Env(lib, track, n_envs=4, n_rays=36) as g:
        base = g.base_dynamics()
        rows = make_rows(base, 4, 3).reshape(4, 1, 8)
        g.set_dynamics(rows)
        before = g.dynamics()
        for car, entry, value in ((2, 1, 0.0), (1, 5, np.inf), (3, 0, np.nan), (0, 2, -0.1)):
            bad = rows.copy()
            bad[car, 0, entry] = value
            try:
                g.set_dynamics(bad)
            except capi.FtgpError as x:
                assert x.code == ERR_ARG and f"car {car}" in str(x) and capi.DYN_FIELDS[entry] in str(x), x
            else:
                raise AssertionError(f"{capi.DYN_FIELDS[entry]} = {value} was accepted")
            after = g.dynamics()
            np.testing.assert_array_equal(after[0], before[0])
            assert after[1] == before[1] == 0
        # a bad row of an env the mask leaves out is not looked at
        bad = rows.copy()
        bad[2, 0, 1] = 0.0
        g.set_dynamics(bad, np.array([1, 1, 0, 1], dtype=np.uint8))
        np.testing.assert_array_equal(g.dynamics()[0], before[0])
    print("errors ok")


def vec_env(opt):
    from ft_grandprix_amd.vec import DeviceVecEnv
    n, bounds = 16, {"friction": (0.3, 0.9), "mass": (4.0, 8.0)}
    kw = dict(n_envs=n, n_rays=64, max_episode_steps=20, randomize_dynamics=bounds, spawn_mode=1, seed=5)
    venv = DeviceVecEnv("small-circle", dynamics_seed=4, **kw)
    other = DeviceVecEnv("small-circle", dynamics_seed=4, **kw)
    third = DeviceVecEnv("small-circle", dynamics_seed=5, **kw)
    torch.cuda.synchronize()
    first = venv.dynamics.cpu().numpy()
    np.testing.assert_array_equal(first, other.dynamics.cpu().numpy())
    assert (first != third.dynamics.cpu().numpy()).any()
    other.close()
    third.close()
    base = venv.env.base_dynamics()
    named = [capi.DYN_FIELDS.index(f) for f in bounds]

    def check_rows(rows, what):
        assert rows.shape == (n, 1, 8) and rows.dtype == np.float64
        for f, (lo, hi) in bounds.items():
            col = rows[:, :, capi.DYN_FIELDS.index(f)]
            assert (col >= lo).all() and (col <= hi).all(), (what, f, col.min(), col.max())
        rest = np.delete(rows, named, axis=2)
        np.testing.assert_array_equal(rest, np.broadcast_to(np.delete(base, named), rest.shape), err_msg=what)
        got, rejected = venv.env.dynamics()
        np.testing.assert_array_equal(rows.reshape(n, 8), got, err_msg=what)
        assert rejected == 0

    check_rows(first, "construction")
    venv.reset()
    torch.cuda.synchronize()
    rows = venv.dynamics.cpu().numpy()
    assert (rows[:, 0, named] != first[:, 0, named]).all(), "reset() draws new rows for every env"
    check_rows(rows, "reset")
    act = torch.tensor([1.5, 0.1], dtype=torch.float32, device=venv.device).repeat(n, 1, 1).contiguous()
    n_ended = 0
    for call in range(50):
        if call == 7:                                 # stagger the episodes: the first half starts again now
            torch.cuda.synchronize()
            venv.env.reset(np.arange(n) < n // 2)
        _, _, te, tr, _ = venv.step(act)
        ended = (te | tr).cpu().numpy()
        new = venv.dynamics.cpu().numpy()
        changed = (new != rows).any(axis=(1, 2))
        np.testing.assert_array_equal(changed, ended, err_msg=f"call {call}: rows change exactly for the envs that ended")
        if ended.any():
            assert (new[ended][:, 0, named] != rows[ended][:, 0, named]).all()
            check_rows(new, f"call {call}")
            n_ended += int(ended.sum())
        rows = new
    assert n_ended == 2 * n, n_ended                      # calls 19 and 39 end one half's episodes, calls 26 and 46 the other's
    assert is_dynamics_kernel(venv.env.kernel_name()), venv.env.kernel_name()
    # rows of the caller's choosing, masked; an invalid one is kept out of the mirror as the library keeps it out of the table
    mine = np.tile(base, (n, 1, 1))
    mine[:, 0, 2] = np.linspace(0.4, 0.8, n)
    mine[3, 0, 0] = -2.0
    mask = torch.zeros(n, dtype=torch.bool, device=venv.device)
    mask[[1, 3, 9]] = True
    venv.set_dynamics(mine, mask)
    torch.cuda.synchronize()
    want = rows.copy()
    want[[1, 9]] = mine[[1, 9]]
    np.testing.assert_array_equal(venv.dynamics.cpu().numpy(), want)
    got, rejected = venv.env.dynamics()
    np.testing.assert_array_equal(got, want.reshape(n, 8))
    assert rejected == 1, rejected
    venv.close()
    print(f"vec env ok: {n_ended} episode ends")


SCENARIOS = {"closed_loop": closed_loop, "multi_car": multi_car, "distinct_rows": distinct_rows, "neutral": neutral,
             "device_setter": device_setter, "multitrack": multitrack, "tricycle": tricycle, "errors": errors, "vec_env": vec_env}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
