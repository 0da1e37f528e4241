"""The free vehicle step -- K1 without its contacts: heading, Ackermann angles, velocity servo and its clamp, tyre slip and the friction
circle, wheel spin, steering servo and its stops, the integrator, the tricycle's torque motors -- against a model that owes nothing
to the oracle or the kernel (tests/free_step_model.py: body frame, libm, statics for the wheel loads; long double).

Protocol, the same for every scene (free_step_model.Scene): an open field without walls, single steps.  Before each step pose() and
ctrl() are read, the model steps from that observable state and its OWN hidden state (wheel spins, steering joint: zero after a reset,
never readable), the library steps, pose() is compared.  Per step and car, on x, y, vx, vy, wz and the heading (qw^2 - qz^2, 2 qw qz):
|library - model| <= 1e-12 max(1, |component before the step|); |qw^2 + qz^2 - 1| <= 4 * 2^-52; the model in binary64 within 1e-13 of
itself in long double.  A hidden quantity that is wrong shows one step later: the model built from a vehicle that differs by 1 % in
any one constant misses by 7e-4 or more (test_a_model_of_a_slightly_different_vehicle_disagrees).

CPU: the oracle.  GPU: libftgp.so, one fresh child process per scenario (tests/free_step_child.py), with an oracle twin on the same
inputs that must equal it bit for bit.
"""
import functools
import os

import numpy as np
import pytest

from ft_grandprix_amd import capi
from tests import children, helpers
from tests import free_step_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "free_step_child.py")
KW = dict(n_rays=8)
N = 6                        # cars of a CPU scene, one per env
TRI_DT = 0.0075
TRI_CTRL = dict(speed=(-6.0, 6.0), steer=(-1.5, 1.5))          # beyond the ctrlrange +-4 / +-1: the clamps act


def vehicle_with(base, row):
    v = capi.FtgpVehicle.from_buffer_copy(base)
    for f, x in zip(capi.DYN_FIELDS, row):
        setattr(v, f, float(x))
    return v


def masked_reset(env, envs):
    def event(scene):
        mask = np.zeros(env.n_envs, dtype=np.uint8)
        mask[envs] = 1
        env.reset(mask)
        scene.reset_cars(np.asarray(envs))
    return event


def cruise(lib):
    with capi.Env(lib, helpers.open_field(), n_envs=N, **KW) as e:
        return fm.Scene([e], fm.vehicle_record(e.cfg.vehicle), seed=1).run(1000)


def kicks(lib):
    with capi.Env(lib, helpers.open_field(), n_envs=N, **KW) as e:
        return fm.Scene([e], fm.vehicle_record(e.cfg.vehicle), seed=2, kick_every=40).run(400)


def reset(lib):
    with capi.Env(lib, helpers.open_field(), n_envs=N, **KW) as e:
        events = {130: masked_reset(e, [1, 4]), 255: masked_reset(e, [0, 1, 5])}
        return fm.Scene([e], fm.vehicle_record(e.cfg.vehicle), seed=3, kick_every=40).run(400, events)


def rows(lib):
    """One handle per vehicle (the oracle has no table); the model is given the default vehicle and the rows."""
    base = lib.default_vehicle()
    base_row = np.array([getattr(base, f) for f in capi.DYN_FIELDS])
    table = base_row * np.random.default_rng(4).uniform(helpers.DYN_LO, helpers.DYN_HI, (5, 8))
    table[0], table[1] = base_row * helpers.DYN_LO, base_row * helpers.DYN_HI
    parts = [capi.Env(lib, helpers.open_field(), n_envs=1, vehicle=vehicle_with(base, r), **KW) for r in table]
    try:
        return fm.Scene(parts, fm.vehicle_record(base), seed=5, rows=table, kick_every=40).run(400)
    finally:
        for p in parts:
            p.close()


def tricycle(lib):
    veh = lib.tricycle_vehicle()
    with capi.Env(lib, helpers.open_field(), n_envs=N, vehicle=veh, dt=TRI_DT, **KW) as e:
        return fm.Scene([e], fm.vehicle_record(veh), seed=6, dt=TRI_DT, kick_every=40, **TRI_CTRL).run(400)


def tricycle_cruise(lib):
    veh = lib.tricycle_vehicle()
    with capi.Env(lib, helpers.open_field(), n_envs=N, vehicle=veh, dt=TRI_DT, **KW) as e:
        return fm.Scene([e], fm.vehicle_record(veh), seed=7, dt=TRI_DT, **TRI_CTRL).run(400)


SCENES = {"cruise": cruise, "kicks": kicks, "reset": reset, "rows": rows, "tricycle": tricycle, "tricycle_cruise": tricycle_cruise}
KIND = {"mushr": ("cruise", "kicks", "reset", "rows"), "tricycle": ("tricycle", "tricycle_cruise")}


@functools.lru_cache(maxsize=None)
def ran(lib, name):
    """Every scene runs once per session; the coverage and mutation tests read what it left."""
    return SCENES[name](lib)


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_free_step_meets_the_model(oracle, name):
    f = ran(oracle, name).report(name)
    assert f["worst"] <= fm.TOL and f["model_gap"] <= fm.MODEL_TOL and f["unit"] <= fm.UNIT_TOL, f


@pytest.mark.parametrize("kind", list(KIND))
def test_scenes_cover_both_tyre_regimes_and_the_clamps(oracle, kind):
    """Counted by the model alone: a scene set that never leaves the friction circle, or never enters it, pins half the tyre."""
    total = {k: sum(ran(oracle, s).figures()[k] for s in KIND[kind]) for k in ("inside", "on", "throttle_clamped", "steer_stop")}
    print(kind, total)
    assert total["inside"] >= 500 and total["on"] >= 500, total
    if kind == "mushr":
        assert total["throttle_clamped"] >= 50 and total["steer_stop"] >= 50, total


def nudged(values, i):
    return [x * 1.01 if k == i else x for k, x in enumerate(values)]


MUTATIONS = [(f, None) for f in capi.DYN_FIELDS] + [(f, None) for f in ("wheel_radius", "wheel_inertia", "wheel_damping", "throttle_gear",
                                                                         "steer_inertia", "steer_limit", "gravity")] + [("wheel_x", 1), ("wheel_y", 2)]


@pytest.mark.parametrize("field,index", MUTATIONS, ids=[f if i is None else f"{f}[{i}]" for f, i in MUTATIONS])
def test_a_model_of_a_slightly_different_vehicle_disagrees(oracle, field, index):
    """The test of the test: the oracle's kicks scene, run on the true vehicle, replayed by the model of a vehicle with one constant
    1 % larger.  More than 1e-6 somewhere (measured: 7e-4 or more) proves that the scene reaches that constant."""
    trace = ran(oracle, "kicks").trace
    true = fm.vehicle_record(oracle.default_vehicle())
    assert fm.replay(trace[:100], true) <= fm.TOL
    value = getattr(true, field)
    wrong = fm.vehicle_record(true, **{field: value * 1.01 if index is None else nudged(value, index)})
    miss = fm.replay(trace, wrong)
    print(f"{field}{'' if index is None else [index]} + 1 %: the model misses by {miss:.2e}")
    assert miss > 1e-6, miss


def test_wheel_loads_balance_the_weight(oracle):
    """The statics of the model itself: the loads sum to m g and their moment about the body origin vanishes, caster included."""
    lib = oracle
    for v in (lib.default_vehicle(), lib.tricycle_vehicle()):
        veh = fm.vehicle_record(v)
        load = fm.FreeStepModel(1).wheel_loads(veh, np.array([veh.mass], dtype=np.longdouble))[0]
        wheels = 3 if veh.kind == fm.TRICYCLE else 4
        assert load[wheels:].sum() == 0 and (load[:wheels] > 0).all()
        assert abs(load.sum() / (veh.mass * veh.gravity) - 1) < 1e-15
        assert abs(sum(load[i] * veh.wheel_x[i] for i in range(wheels))) < 1e-15 * veh.mass * veh.gravity
        assert abs(sum(load[i] * veh.wheel_y[i] for i in range(wheels))) < 1e-15 * veh.mass * veh.gravity


# ---------------------------------------------------------------------------------------------------------------------- GPU
# one fresh process per scenario; each took 2.0 - 2.4 s on an MI355X, the start of torch and the library included (the scene itself under a
# second): 60 s leaves room for a slow start on a busy machine and still ends a hung child soon
run_child = functools.partial(children.run_child, CHILD, timeout=60)


def kernel_of(out):
    return out.rsplit("kernel ", 1)[1].split("\n")[0].strip()


@pytest.mark.gpu
@pytest.mark.parametrize("n_envs", [1, 5, 19])
def test_gpu_plain_one_car_per_env(n_envs):
    """1 and 5 envs: sixteen lanes per car; 19: two full workgroups of 8 car slots and a ragged one of 3."""
    out = run_child("plain", n_envs=n_envs)
    assert "free step ok" in out and kernel_of(out) == "ftgp_step_kernel<false, false, false>", out[-500:]


@pytest.mark.gpu
def test_gpu_per_car_dynamics_rows():
    """19 envs, one distinct row per car, two masked set_dynamics in mid-scene: each car slot's lanes read that slot's record."""
    out = run_child("dyn")
    assert "free step ok" in out and kernel_of(out) == "ftgp_step_kernel<false, false, false, false, true>", out[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("cars_per_env,n_envs", [(3, 2), (8, 1)])
@pytest.mark.parametrize("dyn", [False, True], ids=["plain", "dyn"])
def test_gpu_multi_car_envs(dyn, cars_per_env, n_envs):
    """Two envs of 3 cars, one env of 8; env-mates kept further than 0.5 apart; every car its own row in the DYN form."""
    want = "ftgp_step_kernel<true, false, false, false, true>" if dyn else "ftgp_step_kernel<true, false, false>"
    out = run_child("multi", cars_per_env=cars_per_env, n_envs=n_envs, dyn=dyn)
    assert "free step ok" in out and kernel_of(out) == want, out[-500:]


@pytest.mark.gpu
def test_gpu_roster_form_through_the_device_step():
    out = run_child("device_step")
    assert "free step ok" in out and kernel_of(out) == "ftgp_step_kernel<false, false, true>", out[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("cars_per_env", [1, 3])
def test_gpu_tricycle(cars_per_env):
    out = run_child("tricycle", cars_per_env=cars_per_env)
    want = "ftgp_step_kernel<true, false, false>" if cars_per_env > 1 else "ftgp_step_kernel<false, false, false>"
    assert "free step ok" in out and kernel_of(out) == want, out[-500:]


@pytest.mark.gpu
def test_gpu_multi_track_handle():
    """Two open fields with different pixel sizes in one handle: the free step does not depend on the track block."""
    out = run_child("multitrack")
    assert "free step ok" in out and kernel_of(out) == "ftgp_step_kernel<false, false, false, true>", out[-500:]
