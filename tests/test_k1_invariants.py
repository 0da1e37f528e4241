"""K1 (the reduced planar model that stands in for mujoco.mj_step on template/mushr.em.xml) against figures that follow from the
MJCF itself.  MuJoCo is not available, so these are not parity tests: they pin the model to what the reference's
model file implies, on a wall-free synthetic map, through the C-ABI -- the oracle on CPU, libftgp.so under `-m gpu`.

  steady speed     velocity servo kv = 100 on the mean wheel spin with gear 0.04, 0.25 per wheel, joint damping 0.01
                   (mushr.em.xml:180,191-196,81): 0.01 * 100 * (u - 0.04 w) = 0.01 w  =>  w = 20 u, ground speed r w = 0.6 u
  turning circle   Ackermann polynomials (mushr.em.xml:185-186) on a wheelbase of 0.14825 (mushr.em.xml:124,150) and a track of
                   0.115: at low speed the rear axle runs on a circle of radius L / tan(q) (the polynomials are the Taylor
                   series of the exact inner / outer wheel angles for that radius)
  steering servo   position servo kp = 20 on a joint with damping 3 x 0.1 and a small inertia (mushr.em.xml:78,179): an
                   overdamped second-order lag, poles at -87 / s and -288 / s, no overshoot, 63 % after 11.5 + 3.5 = 15 ms;
                   seen from outside (path curvature) with the car's own yaw and lateral lags on top
  traction         friction 0.5 = max(wheel 0.3, plane 0.5) (mushr.em.xml:69,94): no acceleration above mu g = 4.905
"""
import math

import numpy as np
import pytest

from ft_grandprix_amd import capi
from tests.helpers import open_field

DT = 0.004
L_WHEELBASE = 0.06925 + 0.079          # mushr.em.xml:124,150 (x 0.5 scale)
X_REAR = 0.079                          # body origin ahead of the rear axle


def drive(lib, ctrl_of_env, n_steps, record_every=1):
    """Constant controls per env from rest; returns pose history [n_records, n_envs, 13]."""
    n = len(ctrl_of_env)
    with capi.Env(lib, open_field(), n_envs=n, n_rays=8) as e:
        e.set_ctrl(np.asarray(ctrl_of_env, dtype=np.float64))
        out = [e.pose()]
        for _ in range(n_steps // record_every):
            e.step(record_every)
            out.append(e.pose())
        assert (e.lidar() == -1).all()                      # nothing to see: every ray leaves the map
        return np.array(out)


def speed(p):
    return np.hypot(p[..., 7], p[..., 8])


def check_steady_speed(lib):
    u = np.array([0.5, 1.0, 2.0, 3.0])
    h = drive(lib, [(x, 0.0) for x in u], 2500, record_every=250)
    v = speed(h[-1])
    np.testing.assert_allclose(v, 0.6 * u, rtol=0.01)                         # r * 20 u
    np.testing.assert_allclose(speed(h[-2]), v, rtol=1e-3)                    # settled
    yaw0 = 2 * np.arctan2(h[0, :, 6], h[0, :, 3]); yaw1 = 2 * np.arctan2(h[-1, :, 6], h[-1, :, 3])
    np.testing.assert_allclose(np.angle(np.exp(1j * (yaw1 - yaw0))), 0.0, atol=1e-9)      # straight ahead
    d = h[-1, :, :2] - h[0, :, :2]
    np.testing.assert_allclose(np.arctan2(d[:, 1], d[:, 0]), yaw0, atol=1e-6)  # ... along the heading


def check_turning_circle(lib):
    q = np.array([0.15, 0.3, 0.5, -0.3])
    h = drive(lib, [(0.5, x) for x in q], 3000, record_every=500)
    p = h[-1]
    r_origin = speed(p) / np.abs(p[:, 12])                                    # v / yaw rate
    r_rear = L_WHEELBASE / np.tan(np.abs(q))
    # a few percent of understeer are physical: the outer wheels spin faster, their joint damping (0.01 w, mushr.em.xml:81) drags
    # harder than the inner ones', and that yaw moment has to be held by slip angles -- independent of the speed for viscous
    # tyres.  The circle may be up to 6 % wider than the kinematic one, never tighter.
    kin = np.hypot(r_rear, X_REAR)
    assert (r_origin >= kin * 0.999).all() and (r_origin <= kin * 1.06).all(), (r_origin, kin)
    assert (np.sign(p[:, 12]) == np.sign(q)).all()                            # positive steering turns left (counter-clockwise)
    np.testing.assert_allclose(speed(p), 0.3, rtol=0.05)                      # the wheels average 0.3; the origin runs a slightly different circle


def check_steering_lag(lib):
    # cruise straight at 0.3 units / s, then step the steering target to 0.3 rad and watch the path curvature follow the joint
    with capi.Env(lib, open_field(), n_envs=1, n_rays=8) as e:
        e.set_ctrl(np.array([[0.5, 0.0]])); e.step(1500)
        e.set_ctrl(np.array([[0.5, 0.3]]))
        kappa = []
        for _ in range(150):
            e.step(1)
            p = e.pose()[0]
            kappa.append(p[12] / math.hypot(p[7], p[8]))
    kappa = np.array(kappa)
    final = kappa[-1]
    assert 0.94 <= final * math.hypot(L_WHEELBASE / math.tan(0.3), X_REAR) <= 1.001      # the (slightly understeering) circle of check_turning_circle
    assert kappa.max() <= final * 1.02                                        # overdamped: no overshoot
    t63 = (np.argmax(kappa >= 0.63 * final) + 1) * DT
    t95 = (np.argmax(kappa >= 0.95 * final) + 1) * DT
    # three lags in series: the servo (11.5 + 3.5 ms), the yaw response Izz / sum(c x_i^2) = 0.0317 / 3.26 = 10 ms and the lateral
    # one m / (4 c) = 5.63 / 592 = 10 ms (c = tyre coupling 148 N s / m per wheel): 63 % after about 35 ms
    assert 0.025 <= t63 <= 0.045, t63
    # the last few percent wait for the slowest mode: the inner and outer wheels settling to their own spins,
    # I_w / (r^2 c) = 0.0103 / 0.133 = 77 ms
    assert t95 <= 0.300, t95


def check_traction_limit(lib):
    h = drive(lib, [(7.0, 0.0), (3.0, 0.0), (0.3, 0.0)], 500)                 # `fast` asks for 7 on a straight (fast.py:135-136)
    v = speed(h)
    acc = np.diff(v, axis=0) / DT
    mu_g = 0.5 * 9.81
    assert acc.max() <= mu_g * (1 + 1e-9)
    assert acc[1:50, 0].min() >= 0.98 * mu_g                                  # wheels spinning: the launch sits ON the limit ...
    assert acc[:, 2].max() < 0.5 * mu_g                                       # ... a gentle command never gets near it
    assert v[-1, 0] == pytest.approx(4.2, rel=0.02) or v[-1, 0] < 4.2         # 0.6 * 7 is where it is heading


CHECKS = [check_steady_speed, check_turning_circle, check_steering_lag, check_traction_limit]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_oracle_model_meets_mjcf_figures(oracle, check):
    check(oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_gpu_model_meets_mjcf_figures(product, check):
    check(product)
