"""An independent model of the free vehicle step (K1 without its wall and car-car contacts), written from DESIGN.md section 3 and the
constants a vehicle record carries.  numpy only: no ctypes, no oracle, no library.  tests/test_free_step.py (oracle, CPU) and
tests/free_step_child.py (libftgp.so, GPU) hold the libraries to it.

It is deliberately another formulation than the library's, so that a slip shared by the kernel and the oracle shows:

  heading       yaw = 2 atan2(qz, qw), libm sin / cos of the angles (the library: 1 - 2 qz^2, Taylor polynomials)
  frame         everything in the BODY frame: the velocity is rotated in once, the contact-point velocity is v_b + w x p_i with p_i
                in body coordinates, wheel i points along (cos d_i, sin d_i), the torque is p_i x F_i, the force sum is rotated back
                once at the end (the library: world frame throughout)
  Ackermann     plain power sums q +- 0.375 q^2 + 0.140625 q^3 -+ 0.0722656 q^4 (the library: Horner)
  friction      F min(1, mu N_i / |F|) with hypot (the library: compares squares, scales by lim / sqrt)
  wheel loads   from statics: the moment balance of the weight (at the body origin) about the other axle gives an axle's load, a
                wheel carries half its axle's.  The tricycle's caster is an axle of one wheel that carries its share and transmits
                nothing; there is no fourth wheel.
  attitude      yaw + dt wz', returned as (cos, sin) of half of it (the library: a quaternion product, renormalised)

What the two share is the physics: viscous tyre coupling on the slip velocity, wheel spin and steering servo with implicit damping,
the clamp of the throttle force, the steering stops with the velocity into the stop zeroed, semi-implicit Euler.

The hidden state of a car (four wheel spins, steering angle and rate) cannot be read through the C-ABI.  It is zero after a reset, and
the model integrates it itself: given the controls and the observable state before every step it stays in step with the library, so
a wrong hidden state shows in the observables one step later.
"""
import types

import numpy as np

OBSERVABLES = ("x", "y", "qw", "qz", "vx", "vy", "wz")
POSE_COLUMNS = (0, 1, 3, 6, 7, 8, 12)                # of a 13-double pose row: x, y, qw, qz, vx, vy, wz
DYN_FIELDS = ("mass", "izz", "friction", "tire_damping", "throttle_kv", "throttle_force_limit", "steer_kp", "steer_damping")
SCALARS = ("wheel_radius", "wheel_inertia", "wheel_damping", "throttle_gear", "steer_inertia", "steer_limit", "gravity",
           "motor_forward_limit", "motor_turn_limit")
TRICYCLE = 1                                          # FTGP_VEHICLE_TRICYCLE


def vehicle_record(v, **changes):
    """The fields the free step reads of a vehicle (any object with these attributes) as a plain namespace of Python floats and lists;
    `changes` replace fields (a list for wheel_x / wheel_y)."""
    r = types.SimpleNamespace(kind=int(v.kind), wheel_x=[float(x) for x in v.wheel_x], wheel_y=[float(y) for y in v.wheel_y])
    for f in DYN_FIELDS + SCALARS:
        setattr(r, f, float(getattr(v, f)))
    for f, x in changes.items():
        assert hasattr(r, f), f
        setattr(r, f, x)
    return r


def widen_f32(a):
    """binary32 actions as the binary64 controls they become: every binary32 value is a binary64 value."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def heading(qw, qz):
    """(cos yaw, sin yaw) of the quaternion (qw, 0, 0, qz): what a pose is compared on (q and -q are one attitude)."""
    return qw * qw - qz * qz, 2.0 * qw * qz


class FreeStepModel:
    """n cars; `real` is the arithmetic type of everything, hidden state included."""

    def __init__(self, n_cars, real=np.longdouble):
        self.n, self.real = int(n_cars), real
        self.spin = np.zeros((self.n, 4), dtype=real)          # wheel spins, rad / s
        self.steer = np.zeros(self.n, dtype=real)              # steering joint angle
        self.steer_rate = np.zeros(self.n, dtype=real)
        self.count = dict(inside=0, on=0, throttle_clamped=0, steer_stop=0)

    def reset(self, cars=None):
        """Zero the hidden state of `cars` (a boolean mask or indices; None = all)."""
        k = slice(None) if cars is None else cars
        self.spin[k] = 0
        self.steer[k] = 0
        self.steer_rate[k] = 0

    # ------------------------------------------------------------------------------------------------------------------ statics
    def wheel_loads(self, veh, mass):
        """Static normal force under every wheel position, [n, 4].  The weight m g acts at the body origin (x = 0).  An axle at x_a
        and the other at x_b: moments about the other axle, N_a (x_a - x_b) = m g (0 - x_b)."""
        T = self.real
        weight = mass * T(veh.gravity)
        wx = [T(x) for x in veh.wheel_x]
        out = np.zeros((self.n, 4), dtype=T)
        if veh.kind == TRICYCLE:
            x_driven, x_caster = (wx[0] + wx[1]) / 2, wx[2]
            driven = weight * (0 - x_caster) / (x_driven - x_caster)
            out[:, 0] = out[:, 1] = driven / 2
            out[:, 2] = weight * (0 - x_driven) / (x_caster - x_driven)       # the caster carries this and transmits nothing
        else:
            x_front, x_rear = (wx[0] + wx[1]) / 2, (wx[2] + wx[3]) / 2
            front = weight * (0 - x_rear) / (x_front - x_rear)
            rear = weight * (0 - x_front) / (x_rear - x_front)
            out[:, 0] = out[:, 1] = front / 2
            out[:, 2] = out[:, 3] = rear / 2
        return out

    # ------------------------------------------------------------------------------------------------------------------ one step
    def step(self, pose, ctrl, veh, rows=None, dt=0.004):
        """pose [n, 13] before the step, ctrl [n, 2], veh a vehicle record, rows [n, 8] per-car dynamics (DYN_FIELDS) or None.
        Advances the hidden state; returns the observables after the step, [n, 7] of `real` (OBSERVABLES)."""
        T, n = self.real, self.n
        pose = np.asarray(pose, dtype=np.float64).reshape(n, 13).astype(T)
        ctrl = np.asarray(ctrl, dtype=np.float64).reshape(n, 2).astype(T)
        x, y, qw, qz, vx, vy, wz = (pose[:, k] for k in POSE_COLUMNS)
        if rows is None:
            rows = np.tile([getattr(veh, f) for f in DYN_FIELDS], (n, 1))
        rows = np.asarray(rows, dtype=np.float64).reshape(n, 8).astype(T)
        mass, izz, mu, c_tyre, kv, f_limit, kp, steer_damping = (rows[:, k] for k in range(8))
        dt = T(dt)
        radius, spin_inertia, spin_damping = T(veh.wheel_radius), T(veh.wheel_inertia), T(veh.wheel_damping)
        tri = veh.kind == TRICYCLE
        wheels = (0, 1) if tri else (0, 1, 2, 3)

        yaw = 2 * np.arctan2(qz, qw)
        c, s = np.cos(yaw), np.sin(yaw)
        ub, vb = c * vx + s * vy, -s * vx + c * vy             # velocity of the origin, body frame

        zero = np.zeros(n, dtype=T)
        if tri:
            delta = [zero, zero]
            fwd = np.clip(ctrl[:, 0], -T(veh.motor_forward_limit), T(veh.motor_forward_limit))
            turn = np.clip(ctrl[:, 1], -T(veh.motor_turn_limit), T(veh.motor_turn_limit))
            drive = [(fwd - turn) / 2, (fwd + turn) / 2]       # tendons 0.5 (l + r) and 0.5 (r - l): left, right
        else:
            q = self.steer
            delta = [q + T(0.375) * q**2 + T(0.140625) * q**3 - T(0.0722656) * q**4,
                     q - T(0.375) * q**2 + T(0.140625) * q**3 + T(0.0722656) * q**4, zero, zero]
            mean_spin = self.spin.sum(axis=1) / 4
            force = kv * (ctrl[:, 0] - T(veh.throttle_gear) * mean_spin)
            clamped = np.abs(force) > f_limit
            force = np.where(clamped, np.sign(force) * f_limit, force)
            self.count["throttle_clamped"] += int(clamped.sum())
            drive = [force * T(veh.throttle_gear) / 4] * 4

        load = self.wheel_loads(veh, mass)
        fx_b, fy_b, torque = zero.copy(), zero.copy(), zero.copy()
        new_spin = self.spin.copy()
        for i in wheels:
            px, py = T(veh.wheel_x[i]), T(veh.wheel_y[i])
            cu, cv = ub - wz * py, vb + wz * px                 # v_b + w x p_i
            dx, dy = np.cos(delta[i]), np.sin(delta[i])
            slip_long = cu * dx + cv * dy - radius * self.spin[:, i]
            slip_lat = -cu * dy + cv * dx
            f_long, f_lat = -c_tyre * slip_long, -c_tyre * slip_lat
            size = np.hypot(f_long, f_lat)
            grip = mu * load[:, i]
            sliding = size > grip
            scale = np.where(sliding, grip / np.where(sliding, size, 1), 1)
            self.count["on"] += int(sliding.sum())
            self.count["inside"] += int((~sliding).sum())
            f_long, f_lat = f_long * scale, f_lat * scale
            fx = f_long * dx - f_lat * dy
            fy = f_long * dy + f_lat * dx
            fx_b, fy_b = fx_b + fx, fy_b + fy
            torque = torque + px * fy - py * fx
            new_spin[:, i] = (spin_inertia * self.spin[:, i] + dt * (drive[i] - radius * f_long)) / (spin_inertia + dt * spin_damping)
        self.spin = new_spin

        vx1 = vx + dt * (c * fx_b - s * fy_b) / mass
        vy1 = vy + dt * (s * fx_b + c * fy_b) / mass
        wz1 = wz + dt * torque / izz

        if not tri:
            inertia, stop = T(veh.steer_inertia), T(veh.steer_limit)
            rate = (inertia * self.steer_rate + dt * kp * (ctrl[:, 1] - self.steer)) / (inertia + dt * steer_damping)
            angle = self.steer + dt * rate
            high, low = angle > stop, angle < -stop
            rate = np.where((high & (rate > 0)) | (low & (rate < 0)), 0, rate)
            angle = np.where(high, stop, np.where(low, -stop, angle))
            self.count["steer_stop"] += int((high | low).sum())
            self.steer, self.steer_rate = angle.astype(T), rate.astype(T)

        yaw1 = yaw + dt * wz1
        return np.stack([x + dt * vx1, y + dt * vy1, np.cos(yaw1 / 2), np.sin(yaw1 / 2), vx1, vy1, wz1], axis=1)


def ratios(before, got, want):
    """The criterion's left side per car and component, [n, 7]: |got - want| / max(1, |component before the step|) on x, y, vx, vy, wz
    and, in columns 2 and 3, on the heading (cos yaw, sin yaw), whose scale is 1.  before: pose rows [n, 13]; got, want: [n, 7]."""
    L = np.longdouble
    before, got, want = np.asarray(before, dtype=L)[:, list(POSE_COLUMNS)], np.asarray(got, dtype=L), np.asarray(want, dtype=L)
    out = np.abs(got - want) / np.maximum(1, np.abs(before))
    for k, (g, w) in enumerate(zip(heading(got[:, 2], got[:, 3]), heading(want[:, 2], want[:, 3]))):
        out[:, 2 + k] = np.abs(g - w)
    return out.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# The stepping protocol, the same for every scene and both libraries.  Handles are anything with the methods of capi.Env.
TOL = 1e-12                  # library against model: the project's figure for its binary64 models (walls, crowded envs)
MODEL_TOL = 1e-13            # the model in binary64 against itself in long double: the model must not eat the tolerance
UNIT_TOL = 4 * 2.0**-52      # |qw^2 + qz^2 - 1|


class Twin:
    """A second handle run on the same inputs whose poses must equal the library's bit for bit.  It holds the scene's cars `cars` (in
    its own order) and answers for those at the positions `check` (None: all of them)."""

    def __init__(self, env, cars, check=None):
        self.env, self.cars = env, np.asarray(cars)
        self.check = np.arange(len(self.cars)) if check is None else np.asarray(check)


class Scene:
    """One scene: `parts` are the library's handles, their cars concatenated in order; the model gets `veh` and `rows`."""

    def __init__(self, parts, veh, seed, dt=0.004, rows=None, cpe=1, twins=(), speed=(-2.0, 7.0), steer=(-1.2, 1.2), ctrl_every=25,
                 kick_every=0, homes=None):
        self.parts, self.veh, self.dt, self.rows, self.cpe, self.twins = list(parts), veh, dt, rows, cpe, list(twins)
        self.first = np.cumsum([0] + [p.n_cars for p in self.parts])
        self.n = int(self.first[-1])
        self.rng = np.random.default_rng(seed)
        self.speed, self.steer, self.ctrl_every, self.kick_every = speed, steer, ctrl_every, kick_every
        self.homes = self.pose()[:, 0:2].copy() if homes is None else np.asarray(homes, dtype=np.float64)
        self.kick_at_start = homes is not None
        self.model, self.model64 = FreeStepModel(self.n), FreeStepModel(self.n, np.float64)
        self.worst = self.model_gap = self.unit = 0.0
        self.closest = np.inf
        self.trace = []           # per step: (pose before, controls, pose after, cars reset before this step or None)
        self.pending_reset = None

    # -- the library (overridden where a step is not set_ctrl + step)
    def pose(self):
        return np.concatenate([p.pose() for p in self.parts])

    def read_ctrl(self):
        return np.concatenate([p.ctrl() for p in self.parts])

    def set_ctrl(self, ctrl):
        for p, a, b in zip(self.parts, self.first, self.first[1:]):
            p.set_ctrl(ctrl[a:b])
        for t in self.twins:
            t.env.set_ctrl(ctrl[t.cars])

    def set_pose(self, pose):
        for p, a, b in zip(self.parts, self.first, self.first[1:]):
            p.set_pose(pose[a:b])
        for t in self.twins:
            t.env.set_pose(pose[t.cars])

    def advance(self):
        for p in self.parts:
            p.step(1)
        for t in self.twins:
            t.env.step(1)

    def reset_cars(self, cars):
        """The model's part of a masked reset (the caller resets the handles): hidden state of `cars` to zero."""
        self.model.reset(cars)
        self.model64.reset(cars)
        self.pending_reset = np.asarray(cars).copy()

    # -- the scene
    def kick(self):
        """Every car back to its home position with a random heading (both signs of qw), |v| up to 4 in any direction, |wz| up to 6."""
        r, pose = self.rng, self.pose()
        half = r.uniform(-np.pi, np.pi, self.n)
        v, course = r.uniform(0.0, 4.0, self.n), r.uniform(-np.pi, np.pi, self.n)
        pose[:, 0:2] = self.homes
        pose[:, 3], pose[:, 6] = np.cos(half), np.sin(half)
        pose[:, 7], pose[:, 8], pose[:, 12] = v * np.cos(course), v * np.sin(course), r.uniform(-6.0, 6.0, self.n)
        self.set_pose(pose)

    def run(self, steps, events=None, check=True):
        events = events or {}
        for k in range(steps):
            if k in events:
                events[k](self)
            if self.kick_every and k % self.kick_every == 0 and (k > 0 or self.kick_at_start):
                self.kick()
            if k % self.ctrl_every == 0:
                self.set_ctrl(np.stack([self.rng.uniform(*self.speed, self.n), self.rng.uniform(*self.steer, self.n)], axis=1))
            before, ctrl = self.pose(), self.read_ctrl()
            want = self.model.step(before, ctrl, self.veh, self.rows, self.dt)
            want64 = self.model64.step(before, ctrl, self.veh, self.rows, self.dt)
            self.advance()
            after = self.pose()
            self.trace.append((before, ctrl, after, self.pending_reset))
            self.pending_reset = None
            for t in self.twins:
                np.testing.assert_array_equal(after[t.cars[t.check]], t.env.pose()[t.check], err_msg=f"step {k}: the library and its oracle twin")
            if self.cpe > 1:
                xy = after[:, 0:2].reshape(-1, self.cpe, 2)
                d = np.hypot(*(xy[:, :, None, :] - xy[:, None, :, :]).transpose(3, 0, 1, 2)) + np.where(np.eye(self.cpe), np.inf, 0.0)
                self.closest = min(self.closest, float(d.min()))
                assert d.min() >= 0.5, f"step {k}: env-mates {d.min()} apart: a contact could couple them"
            r = ratios(before, after[:, list(POSE_COLUMNS)], want)
            gap = ratios(before, want64, want)
            unit = np.abs(after[:, 3].astype(np.longdouble)**2 + after[:, 6].astype(np.longdouble)**2 - 1)
            self.worst, self.model_gap, self.unit = max(self.worst, float(r.max())), max(self.model_gap, float(gap.max())), max(self.unit, float(unit.max()))
            if check:
                car, comp = np.unravel_index(r.argmax(), r.shape)
                name = ("x", "y", "cos yaw", "sin yaw", "vx", "vy", "wz")[comp]
                assert r.max() <= TOL, (f"step {k}, car {car}, {name}: |library - model| / scale = {r.max():.3e} > {TOL}\nbefore {before[car]}\n"
                                        f"controls {ctrl[car]}\nlibrary {after[car]}\nmodel {want[car]}")
                assert gap.max() <= MODEL_TOL, f"step {k}: the model in binary64 is {gap.max():.3e} from itself in long double"
                assert unit.max() <= UNIT_TOL, f"step {k}: |qw^2 + qz^2 - 1| = {unit.max():.3e}"
        return self

    def figures(self):
        c = self.model.count
        return dict(worst=self.worst, model_gap=self.model_gap, unit=self.unit, steps=len(self.trace), cars=self.n, **c)

    def report(self, name):
        f = self.figures()
        line = (f"{name}: {f['cars']} cars x {f['steps']} steps, worst |library - model| / scale {f['worst']:.2e}, binary64 model vs long double "
                f"{f['model_gap']:.2e}, |q|^2 - 1 {f['unit']:.1e}; wheel evaluations inside / on the circle {f['inside']} / {f['on']}, "
                f"throttle clamped {f['throttle_clamped']}, at a steering stop {f['steer_stop']}")
        if self.cpe > 1:
            line += f", env-mates never closer than {self.closest:.2f}"
        print(line)
        return f


def replay(trace, veh, rows=None, dt=0.004, real=np.longdouble):
    """A model of `veh` over the recorded steps of a scene (resynchronised before every step as in the scene): the worst ratio."""
    model = FreeStepModel(len(trace[0][0]), real)
    worst = 0.0
    for before, ctrl, after, reset in trace:
        if reset is not None:
            model.reset(reset)
        worst = max(worst, float(ratios(before, after[:, list(POSE_COLUMNS)], model.step(before, ctrl, veh, rows, dt)).max()))
    return worst


def grid_homes(n_envs, cpe, centre=(20.0, -20.0), pitch=3.0):
    """Home positions [n_envs * cpe, 2] for envs of `cpe` cars: the cars of an env on a 3 x 3 grid `pitch` apart (envs share the
    ground: cars of different envs do not see each other).  Between two kicks, 40 steps, a car moves |v| t + a t^2 / 2 at the most,
    with |v| <= 4 after a kick and a <= mu g: 0.70 in 0.16 s for the MuSHR car (mu 0.5), 1.64 in 0.3 s for the tricycle (mu 1), so a
    pitch of 3 resp. 4.5 keeps env-mates more than 0.5 apart; the scene asserts it from the poses."""
    assert cpe <= 9
    cell = np.array([(i % 3 - 1, i // 3 - 1) for i in range(cpe)], dtype=np.float64) * pitch
    return np.tile(np.asarray(centre) + cell, (n_envs, 1))
