"""What the children of the device-step tests share (tests/device_io_child.py, device_signals_child.py, device_contacts_child.py,
device_frame_child.py, spawn_rule_child.py): the host twin of a DeviceVecEnv -- handle B on the host path and, from its read-backs alone,
what a device call on handle A must have written (tests/signals_model.py, tests/contacts_model.py) --, the events that both handles
get alike (teleport, push_off), the torch driver, and `refused`.  Nothing here loads the library or imports torch: the children do.
"""
import numpy as np

from ft_grandprix_amd import capi
from tests import contacts_model as cm
from tests import signals_model as sm


def _spawn_point(env, car):
    return (10 + 7 * env + 2 * car) % 98          # spawn_mode 1 (ftgp_reset_kernel)


def _same_pose(handles):
    pose = handles[0].pose()
    for h in handles[1:]:
        np.testing.assert_array_equal(h.pose(), pose)
    return pose


def _apply(handles, pose):
    for h in handles:
        h.set_pose(pose)
        h.eval_progress()


def teleport(handles, paths, envs, cars, cpe, rolling=True):
    """The given cars, on every handle alike, to the last centre-line point of their lap (through 40 % and 80 % of it, so that the
    progress rule counts no crossing): a short drive forward then finishes the lap.  rolling: they roll along the line at 3 units/s;
    without it their velocities are left as they are.  ftgp_set_pose + ftgp_eval_progress: host calls that all handles make identically."""
    pose = _same_pose(handles)
    for frac in (40, 80, 99):
        for e in envs:
            for c in cars:
                path = paths[e]
                q = (_spawn_point(e, c) + frac) % 100
                a = np.arctan2(path[(q + 1) % 100, 1] - path[q, 1], path[(q + 1) % 100, 0] - path[q, 0])
                row = pose[e * cpe + c]
                row[0], row[1], row[3], row[6] = path[q, 0], path[q, 1], np.cos(a / 2), np.sin(a / 2)
                if rolling:
                    row[7], row[8], row[12] = 3.0 * np.cos(a), 3.0 * np.sin(a), 0.0
        _apply(handles, pose)


def push_off(handles, paths, envs, cars, cpe, dist=1.5):
    """The given cars, on every handle alike, `dist` units off the centre-line, along the normal at the point nearest to them."""
    pose = _same_pose(handles)
    for e in envs:
        for c in cars:
            path, row = paths[e], pose[e * cpe + c]
            q = int(((path - row[0:2]) ** 2).sum(axis=1).argmin())
            t = path[(q + 1) % 100] - path[(q - 1) % 100]
            n = np.array([-t[1], t[0]]) / np.hypot(t[0], t[1])
            row[0], row[1] = path[q, 0] + dist * n[0], path[q, 1] + dist * n[1]
    _apply(handles, pose)


class HostTwin:
    """Handle B and what a device call must have written, from its host read-backs."""

    def __init__(self, B, roster, paths, pool, M, penalty, term_off, max_steps, repeat, auto_reset, dist2_of=None):
        self.B, self.roster, self.cpe = B, roster, len(roster)
        self.ext = [k for k, r in enumerate(roster) if r == "agent"]
        self.bundled = len(self.ext) < self.cpe
        self.car_paths = np.repeat(np.asarray(paths), self.cpe, axis=0)          # [n_cars, 100, 2]
        self.pool, self.M, self.penalty, self.term_off = pool, M, np.float32(penalty), term_off
        self.max_steps, self.repeat, self.auto_reset = max_steps, repeat, auto_reset
        self.dist2_of = dist2_of or (lambda b: b.centre_dist2())
        self.n = B.n_envs
        self.car_mask = np.zeros((self.n, self.cpe), dtype=np.uint8)
        self.car_mask[:, self.ext] = 1
        self.count = dict(off_term=0, fin_term=0, trunc=0, clipped=0, mixed=0, all_miss=0, penalised=0)
        if self.bundled:
            B.set_car_policies(["lobotomy" if r == "agent" else r for r in roster])

    def _ext(self, x):
        return x.reshape((self.n, self.cpe) + x.shape[1:])[:, self.ext]

    def state(self):
        B = self.B
        d2, pose, prog = self.dist2_of(B), B.pose(), B.progress()
        racing = prog[:, 4] == 0
        # the stored field is the model's value, to the bit: the same subtractions, squares, sum and comparisons (no fused operation)
        np.testing.assert_array_equal(d2[racing], sm.centre_dist2(pose, self.car_paths)[racing], err_msg="centre_dist2 against numpy")
        return self._ext(sm.state_rows(pose, B.ctrl(), prog, d2))

    def call(self, a):
        """One device call on B with actions a float64 [n_envs, n_ext, 2]; returns what A must hold."""
        B, n, cpe, ext = self.B, self.n, self.cpe, self.ext
        p0 = B.progress()
        for _ in range(self.repeat):
            fin = B.progress()[:, 4].reshape(n, cpe)
            ctrl = np.zeros((n, cpe, 2), dtype=np.float64)
            if self.bundled:
                ctrl = B.policy_eval("per_car", B.lidar()).reshape(n, cpe, 2)
            ctrl[:, ext] = np.where(fin[:, ext, None] != 0, 0.0, a)
            B.set_ctrl(ctrl, self.car_mask if self.bundled else None)
            B.step(1)
        p1 = B.progress()
        off = self._ext(p1[:, 5]) != 0
        reward = self._ext(p1[:, 3] - p0[:, 3]).astype(np.float32)
        reward = np.where(off, reward - self.penalty, reward).astype(np.float32)
        fin_all = (self._ext(p1[:, 4]) != 0).all(axis=1)
        term = fin_all | (bool(self.term_off) & off.any(axis=1))
        trunc = ~term & (self.max_steps > 0) & (B.steps() >= self.max_steps)
        lid = self._ext(B.lidar())
        obs = sm.pool_scan(lid, self.pool, self.M)
        state = self.state()
        ended = term | trunc
        out = dict(reward=reward, terminated=term, truncated=trunc, ended=ended, off=off, final_obs=None, final_state=None)
        if self.auto_reset and ended.any():
            out["final_obs"], out["final_state"] = obs[ended].copy(), state[ended].copy()
            B.reset(ended.astype(np.uint8))
            obs[ended] = 0.0
            state = self.state()                  # the spawn state of the envs just reset; the others' rows are what they were
        out["obs"], out["state"] = obs, state
        c = self.count
        c["off_term"] += int((term & ~fin_all).sum()); c["fin_term"] += int(fin_all.sum()); c["trunc"] += int(trunc.sum())
        mixed, all_miss, clipped = sm.beam_classes(lid, self.pool, self.M)
        c["mixed"] += mixed; c["all_miss"] += all_miss; c["clipped"] += clipped; c["penalised"] += int(off.sum())
        return out


def torch_driver(torch, obs, gen, dev):
    """The driver of the device-step children on whatever the observation holds: steer towards the largest value of the front half,
    speed ~ U(0.5, 3); then noise, some of it past the ctrlrange."""
    n, k, nb = obs.shape
    front = obs[:, :, nb // 4: 3 * nb // 4]
    j = front.argmax(dim=2).float() / max(1, front.shape[2] - 1)
    steer = (j - 0.5) * 2.0
    speed = 0.5 + 2.5 * torch.rand((n, k), generator=gen, device=dev)
    act = torch.stack([speed, steer + 0.3 * torch.randn((n, k), generator=gen, device=dev)], dim=2)
    wild = torch.rand((n, k, 2), generator=gen, device=dev) < 0.05
    return torch.where(wild, 6.0 * torch.randn((n, k, 2), generator=gen, device=dev), act).contiguous()


def _tracks(opt):
    from ft_grandprix_amd.track import load_track
    names = opt.get("track", "small-circle")
    multi = isinstance(names, list)
    tracks = [sm.open_right_track() if t == "open-right" else load_track(t) for t in (names if multi else [names])]
    return (tracks if multi else tracks[0]), tracks


def _full_state(env):
    counts, times = env.lap_times()
    return dict(pose=env.pose(), progress=env.progress(), lap_counts=counts, lap_times=times, steps=env.steps(), lidar=env.lidar(),
                ctrl=env.ctrl(), dist2=env.centre_dist2(), race_steps=env.race_steps())


def _same_state(A, B):
    a, b = _full_state(A), _full_state(B)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"handle state at the end: {k}")


class ContactTwin(HostTwin):
    """HostTwin with the contact rules of include/ftgp.h on top."""

    def __init__(self, B, roster, paths, tracks, envs_per_track, vehicle, con, **kw):
        super().__init__(B, roster, paths, **kw)
        self.tracks, self.envs_per_track, self.vehicle = tracks, envs_per_track, vehicle
        self.term_wall, self.term_car = con["terminate_on_wall"], con["terminate_on_car"]
        self.wall_penalty, self.car_penalty = np.float32(con["wall_penalty"]), np.float32(con["car_penalty"])
        self.count.update(wall_term=0, car_term=0, wall_penalised=0, car_penalised=0, final_wall=0, final_car=0, wall_rows=0, car_rows=0)

    def contacts(self):
        B = self.B
        rows = cm.contact_rows_blocks(self.tracks, self.envs_per_track, self.vehicle, B.pose(), B.progress()[:, 4], self.cpe, False)
        return self._ext(rows)

    def call(self, a):
        B, n, cpe, ext = self.B, self.n, self.cpe, self.ext
        p0 = B.progress()
        for _ in range(self.repeat):
            fin = B.progress()[:, 4].reshape(n, cpe)
            ctrl = np.zeros((n, cpe, 2), dtype=np.float64)
            if self.bundled:
                ctrl = B.policy_eval("per_car", B.lidar()).reshape(n, cpe, 2)
            ctrl[:, ext] = np.where(fin[:, ext, None] != 0, 0.0, a)
            B.set_ctrl(ctrl, self.car_mask if self.bundled else None)
            B.step(1)
        p1 = B.progress()
        contact = self.contacts()                                   # at the pose after the call's steps, before any reset
        wall, car = contact[:, :, cm.WALL_COUNT] > 0, contact[:, :, cm.CAR_COUNT] > 0
        off = self._ext(p1[:, 5]) != 0
        reward = self._ext(p1[:, 3] - p0[:, 3]).astype(np.float32)
        reward = np.where(off, reward - self.penalty, reward).astype(np.float32)
        reward = np.where(wall, reward - self.wall_penalty, reward).astype(np.float32)
        reward = np.where(car, reward - self.car_penalty, reward).astype(np.float32)
        fin_all = (self._ext(p1[:, 4]) != 0).all(axis=1)
        old = fin_all | (bool(self.term_off) & off.any(axis=1))
        by_wall, by_car = bool(self.term_wall) & wall.any(axis=1), bool(self.term_car) & car.any(axis=1)
        term = old | by_wall | by_car
        trunc = ~term & (self.max_steps > 0) & (B.steps() >= self.max_steps)
        lid = self._ext(B.lidar())
        obs = sm.pool_scan(lid, self.pool, self.M)
        state = self.state()
        ended = term | trunc
        out = dict(reward=reward, terminated=term, truncated=trunc, ended=ended, off=off, by_wall=by_wall, by_car=by_car,
                   final_obs=None, final_state=None, final_contact=None)
        c = self.count
        if self.auto_reset and ended.any():
            out["final_obs"], out["final_state"], out["final_contact"] = obs[ended].copy(), state[ended].copy(), contact[ended].copy()
            c["final_wall"] += int(wall[ended].sum()); c["final_car"] += int(car[ended].sum())
            B.reset(ended.astype(np.uint8))
            obs[ended] = 0.0
            contact = contact.copy()
            contact[ended] = 0.0
            state = self.state()
        out["obs"], out["state"], out["contact"] = obs, state, contact
        c["wall_term"] += int((by_wall & ~old).sum()); c["car_term"] += int((by_car & ~old & ~by_wall).sum())
        c["off_term"] += int((term & ~fin_all & off.any(axis=1)).sum()); c["fin_term"] += int(fin_all.sum()); c["trunc"] += int(trunc.sum())
        c["wall_rows"] += int(wall.sum()); c["car_rows"] += int(car.sum())
        c["wall_penalised"] += int(wall.sum()) if self.wall_penalty > 0 else 0
        c["car_penalised"] += int(car.sum()) if self.car_penalty > 0 else 0
        c["penalised"] += int(off.sum())
        return out


def refused(code, what, f, *a, **k):
    try:
        f(*a, **k)
    except capi.FtgpError as x:
        assert x.code == code, (what, x)
    else:
        raise AssertionError(f"{what} was accepted")
