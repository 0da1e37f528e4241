"""Child process of tests/test_free_step.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/free_step_child.py <scenario> [json options]

Every scenario is the kicks scene of tests/test_free_step.py (free_step_model.Scene: 300 single steps, controls redrawn every 25,
a set_pose kick every 40) with libftgp.so as the library, held to the model by the same 1e-12 criterion, and with oracle twins on
the same inputs whose 13 pose doubles must equal the library's after every step.  The last line names the kernel that ran.
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
from tests import helpers  # noqa: E402
from tests import free_step_model as fm  # noqa: E402

STEPS = 300
KW = dict(n_rays=8)
TRI_DT = 0.0075
TRI_CTRL = dict(speed=(-6.0, 6.0), steer=(-1.5, 1.5))


def vehicle_with(base, row):
    v = capi.FtgpVehicle.from_buffer_copy(base)
    for f, x in zip(capi.DYN_FIELDS, row):
        setattr(v, f, float(x))
    return v


def make_rows(base, n, seed):
    return base * np.random.default_rng(seed).uniform(helpers.DYN_LO, helpers.DYN_HI, (n, 8))


def done(scene, g, what, twins):
    name = g.kernel_name()
    scene.report(what)
    for t in twins:
        t.env.close()
    print(f"free step ok: {what}, kernel {name}")


def plain(opt):
    lib, ora = helpers.libs()
    n = int(opt["n_envs"])
    with capi.Env(lib, helpers.open_field(), n_envs=n, **KW) as g:
        twins = [fm.Twin(capi.Env(ora, helpers.open_field(), n_envs=n, **KW), np.arange(n))]
        scene = fm.Scene([g], fm.vehicle_record(g.cfg.vehicle), seed=20 + n, kick_every=40, twins=twins).run(STEPS)
        done(scene, g, f"plain, {n} envs", twins)


def dyn(opt):
    """One row per car.  Step 100: envs 2, 7 and 18 are reset and get new rows (their twins start again with the new vehicle, so the
    bit-for-bit comparison goes on).  Step 200: envs 0, 8 and 16 get new rows in full motion; an oracle handle cannot follow that (its
    vehicle is fixed, its hidden state cannot be set), so from there on those three are held by the model alone."""
    lib, ora = helpers.libs()
    n, field = 19, helpers.open_field()
    with capi.Env(lib, field, n_envs=n, **KW) as g:
        base = g.base_dynamics()
        rows, later = make_rows(base, n, 31), make_rows(base, n, 32)
        g.set_dynamics(rows.reshape(n, 1, 8))

        def twin(e, row):
            return fm.Twin(capi.Env(ora, field, n_envs=1, env_base=e, vehicle=vehicle_with(g.cfg.vehicle, row), **KW), [e])
        twins = [twin(e, rows[e]) for e in range(n)]
        scene = fm.Scene([g], fm.vehicle_record(g.cfg.vehicle), seed=33, rows=rows.copy(), kick_every=40, twins=twins)

        def change(envs, with_reset):
            def event(s):
                mask = np.zeros(n, dtype=np.uint8)
                mask[envs] = 1
                if with_reset:
                    g.reset(mask)
                    s.reset_cars(np.asarray(envs))
                g.set_dynamics(later.reshape(n, 1, 8), mask)
                got, rejected = g.dynamics()
                want = s.rows.copy()
                want[envs] = later[envs]
                np.testing.assert_array_equal(got, want)
                assert rejected == 0
                s.rows = got                       # the model follows the read-back
                for e in envs:
                    old = next(t for t in s.twins if t.cars[0] == e)
                    old.env.close()
                    s.twins.remove(old)
                    if with_reset:
                        s.twins.append(twin(e, later[e]))
            return event
        scene.run(STEPS, {100: change([2, 7, 18], True), 200: change([0, 8, 16], False)})
        assert len(scene.twins) == n - 3
        assert (g.dynamics()[0] != rows).any(axis=1).sum() == 6
        done(scene, g, "per-car dynamics rows, 19 envs, two masked set_dynamics", scene.twins)


def multi(opt):
    lib, ora = helpers.libs()
    cpe, n, with_rows = int(opt["cars_per_env"]), int(opt["n_envs"]), bool(opt["dyn"])
    field = helpers.open_field()
    kw = dict(cars_per_env=cpe, **KW)
    with capi.Env(lib, field, n_envs=n, **kw) as g:
        rows = None
        if with_rows:                              # every car its own row; twin a has the whole env on row a and answers for car a
            rows = make_rows(g.base_dynamics(), n * cpe, 41)
            g.set_dynamics(rows.reshape(n, cpe, 8))
            twins = [fm.Twin(capi.Env(ora, field, n_envs=1, env_base=a // cpe, vehicle=vehicle_with(g.cfg.vehicle, rows[a]), **kw),
                             np.arange(cpe) + a // cpe * cpe, [a % cpe]) for a in range(n * cpe)]
        else:
            twins = [fm.Twin(capi.Env(ora, field, n_envs=n, **kw), np.arange(n * cpe))]
        scene = fm.Scene([g], fm.vehicle_record(g.cfg.vehicle), seed=42 + cpe, rows=rows, cpe=cpe, kick_every=40, twins=twins,
                         homes=fm.grid_homes(n, cpe)).run(STEPS)
        assert scene.closest >= 0.5
        done(scene, g, f"{n} envs of {cpe} cars, {'one row per car' if with_rows else 'plain'}", twins)


class DeviceStepScene(fm.Scene):
    """A step is one ftgp_step_device call (action_repeat 1) on binary32 actions; the controls the model takes are the model's own
    widening of them, which ctrl() must show after the call."""

    def __init__(self, g, *a, **kw):
        self.g, dev = g, torch.device("cuda", 0)
        n = g.n_envs
        self.obs = torch.zeros((n, 1, g.n_rays), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        self.term, self.trunc = torch.zeros(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.bool, device=dev)
        self.act = torch.zeros((n, 1, 2), dtype=torch.float32, device=dev)
        super().__init__([g], *a, **kw)

    def set_ctrl(self, ctrl):
        a = ctrl.astype(np.float32)
        self.act = torch.from_numpy(a.reshape(-1, 1, 2)).to(self.act.device).contiguous()
        self.widened = fm.widen_f32(a)
        torch.cuda.synchronize()

    def read_ctrl(self):
        return self.widened

    def advance(self):
        self.g.step_device(self.act.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.term.data_ptr(), self.trunc.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(self.g.ctrl(), self.widened)
        assert not self.term.any().item() and not self.trunc.any().item()
        for t in self.twins:
            t.env.set_ctrl(self.widened[t.cars])
            t.env.step(1)


def device_step(opt):
    lib, ora = helpers.libs()
    n, field = 5, helpers.open_field()
    with capi.Env(lib, field, n_envs=n, **KW) as g:
        g.device_io_config(None, max_episode_steps=1_000_000, action_repeat=1, auto_reset=True)    # no episode ends inside the scene
        twins = [fm.Twin(capi.Env(ora, field, n_envs=n, **KW), np.arange(n))]
        scene = DeviceStepScene(g, fm.vehicle_record(g.cfg.vehicle), seed=51, kick_every=40, twins=twins).run(STEPS)
        done(scene, g, "device step, 5 envs", twins)


def tricycle(opt):
    lib, ora = helpers.libs()
    cpe = int(opt["cars_per_env"])
    n, field, veh = (4 if cpe == 1 else 2), helpers.open_field(), lib.tricycle_vehicle()
    kw = dict(n_envs=n, cars_per_env=cpe, vehicle=veh, dt=TRI_DT, **KW)
    with capi.Env(lib, field, **kw) as g:
        twins = [fm.Twin(capi.Env(ora, field, **kw), np.arange(n * cpe))]
        homes = fm.grid_homes(n, cpe, pitch=4.5) if cpe > 1 else None
        scene = fm.Scene([g], fm.vehicle_record(veh), seed=61 + cpe, dt=TRI_DT, cpe=cpe, kick_every=40, twins=twins, homes=homes,
                         **TRI_CTRL).run(STEPS)
        done(scene, g, f"tricycle, {n} envs of {cpe}", twins)


def multitrack(opt):
    lib, ora = helpers.libs()
    tracks, counts = [helpers.open_field(800), helpers.open_field(500)], (2, 2)
    with capi.Env(lib, tracks, n_envs=4, envs_per_track=counts, **KW) as g:
        twins = [fm.Twin(capi.Env(ora, tracks[t], n_envs=2, env_base=2 * t, **KW), np.arange(2) + 2 * t) for t in range(2)]
        scene = fm.Scene([g], fm.vehicle_record(g.cfg.vehicle), seed=71, kick_every=40, twins=twins).run(STEPS)
        done(scene, g, "two-track handle, 4 envs", twins)


SCENARIOS = {"plain": plain, "dyn": dyn, "multi": multi, "device_step": device_step, "tricycle": tricycle, "multitrack": multitrack}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
