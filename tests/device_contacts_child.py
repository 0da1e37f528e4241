"""Child process of tests/test_device_contacts.py: one scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/device_contacts_child.py <scenario> [json options]

`static`: poses put with set_pose; ftgp_get_contacts and ftgp_contacts_device against the numpy model of the header
(tests/contacts_model.py), bit for bit.
`twin`: a DeviceVecEnv with contacts (handle A) against a twin handle B on the host path, bit for bit at every call, after `twin` of
tests/device_signals_child.py (the twins: tests/device_twin.py).  What A must write is modelled from B's host read-backs alone -- the contact rows from pose() and
progress() -- so every count a scenario asserts (`need`) is a count of B's data.
`off`, `zero`, `errors`: contacts off is the old call; a struct of zeros writes rows and changes nothing else; what must be refused.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library is loaded)

from tests import contacts_model as cm  # noqa: E402
from tests import crowded_model as TC  # noqa: E402
from tests import walls_model as TW  # noqa: E402
from tests.device_twin import ContactTwin, _apply, _same_pose, _same_state, _tracks, push_off, refused, teleport, torch_driver  # noqa: E402
from tests.helpers import open_field  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------ static scenes
def static(opt):
    from ft_grandprix_amd import capi
    lib = capi.load()
    roster = opt.get("roster")
    if "scene" in opt:
        sc = TW.contact_scene(opt["scene"])
        v, cpe, bubble, tracks = TW.vehicle_of(lib, sc), sc.cpe, sc.bubble, sc.tracks
        e = TW.contact_env(lib, sc, tracks)
        TW.prepare(e, sc)
        what = opt["scene"]
    else:
        cpe, _, half_width, n_envs, seed = opt["pile_up"]
        v, bubble, tracks = lib.default_vehicle(), False, [open_field()]
        pos, yaw = TC.thrown(cpe, half_width, n_envs, seed)
        e = capi.Env(lib, tracks[0], n_envs=n_envs, cars_per_env=cpe, n_rays=8)
        e.set_pose(TW.put(e.pose(), pos, yaw))
        what = f"pile-up of {cpe}"
    with e:
        pose, done = e.pose(), e.progress()[:, 4] != 0
        n, n_envs = len(pose), len(pose) // cpe
        want = cm.contact_rows_blocks(tracks, capi.split_envs(n_envs, len(tracks)), v, pose, done, cpe, bubble)
        got = e.contacts()
        np.testing.assert_array_equal(got, want, err_msg=f"{what}: ftgp_get_contacts against the model")
        ext = [k for k in range(cpe) if roster is None or roster[k] == "agent"]
        e.device_io_config(roster, 0, 1, True)
        buf = torch.full((n_envs, len(ext), cm.CONTACT_FLOATS), -7.0, dtype=torch.float32, device="cuda:0")
        e.contacts_device(buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(buf.cpu().numpy(), want.reshape(n_envs, cpe, -1)[:, ext], err_msg=f"{what}: ftgp_contacts_device against the model")
        np.testing.assert_array_equal(e.pose(), pose)
        np.testing.assert_array_equal(e.contacts(), want)
        racing = int((~done).sum())
        walls, cars, many = int((want[:, 2] > 0).sum()), int((want[:, 3] > 0).sum()), int((want[:, 3] >= 2).sum())
        print(f"{what}: {n} cars, {n - racing} finished; {walls} touch a wall (most circles {int(want[:, 2].max())}), {cars} overlap a mate, "
              f"{many} two or more; deepest {want[:, 0].max():.4f} / {want[:, 1].max():.4f}")
        assert not want[done].any()
        if "scene" in opt:
            assert 4 * walls >= racing, "the scene shows too few wall contacts"
        else:
            assert 4 * cars >= racing and (cpe <= 2 or many > 0), "the scene shows too few car contacts"
            if roster is not None:
                assert (want.reshape(n_envs, cpe, -1)[:, ext, 3] > 0).any() and len(ext) < cpe
    print("static ok")


# ------------------------------------------------------------------------------------------------------------------ the twin
def wall_centres(track):
    wy, wx = np.nonzero(track.wall_mask())
    return np.stack([track.origin_x + (wx + 0.5) * track.px_size_x, track.origin_y - (wy + 0.5) * track.px_size_y], axis=1)


def push_into_walls(handles, centres, envs, cars, cpe):
    """The given cars, on every handle alike, onto the centre of the wall pixel nearest to them, at rest."""
    pose = _same_pose(handles)
    for e in envs:
        for c in cars:
            row, w = pose[e * cpe + c], centres[e]
            row[0:2] = w[int(((w - row[0:2]) ** 2).sum(axis=1).argmin())]
            row[7:] = 0.0
    _apply(handles, pose)


def nose_to_tail(handles, envs, behind, ahead, cpe, gap=0.18):
    """Car `behind` of the given envs, on every handle alike, `gap` behind car `ahead` on its axis, with its heading and velocity: the
    front circle of the one overlaps the rear circle of the other."""
    pose = _same_pose(handles)
    for e in envs:
        a, b = pose[e * cpe + ahead], pose[e * cpe + behind]
        yaw = 2.0 * np.arctan2(a[6], a[3])
        b[:] = a
        b[0], b[1] = a[0] - gap * np.cos(yaw), a[1] - gap * np.sin(yaw)
    _apply(handles, pose)


def twin(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.vec import DeviceVecEnv
    n_envs, n_rays, cpe = opt.get("n_envs", 64), opt.get("n_rays", 8), opt.get("cars_per_env", 1)
    roster = opt.get("roster", ["agent"] * cpe)
    cpe = len(roster)
    pool, M, state_on = opt.get("pool", 1), opt.get("M", 0.0), opt.get("state", False)
    pen, term_off = opt.get("off_track_penalty", 0.0), opt.get("terminate_off_track", False)
    con = dict(terminate_on_wall=opt.get("terminate_on_wall", False), terminate_on_car=opt.get("terminate_on_car", False),
               wall_penalty=opt.get("wall_penalty", 0.0), car_penalty=opt.get("car_penalty", 0.0))
    R, max_steps, AR = opt.get("action_repeat", 1), opt.get("max_episode_steps", 150), opt.get("auto_reset", True)
    calls, side, epb, push = opt.get("calls", 300), opt.get("side_stream", False), opt.get("envs_per_track"), opt.get("push", "walls")
    kw = dict(lap_target=1, spawn_mode=1, seed=7)
    track, tracks = _tracks(opt)
    if epb is not None:
        kw["envs_per_track"] = epb
    lib, dev = capi.load(), torch.device("cuda", 0)
    venv = DeviceVecEnv(track, n_envs=n_envs, n_rays=n_rays, cars_per_env=cpe, roster=roster, max_episode_steps=max_steps,
                        action_repeat=R, auto_reset=AR, device_id=0, scan_pool=pool, scan_max_range=M, state=state_on,
                        terminate_off_track=term_off, off_track_penalty=pen, contacts=True,
                        terminate_on_wall_contact=con["terminate_on_wall"], terminate_on_car_contact=con["terminate_on_car"],
                        wall_contact_penalty=con["wall_penalty"], car_contact_penalty=con["car_penalty"], **kw)
    A = venv.env
    assert tuple(venv.contact.shape) == (n_envs, roster.count("agent"), 4) and venv.contacts
    B = capi.Env(lib, track, n_envs=n_envs, cars_per_env=cpe, n_rays=n_rays, **kw)
    handles = [A, B]
    paths = [np.asarray(tracks[t].path, dtype=np.float64) for t in B.track_of_env]
    centres = [wall_centres(t) for t in tracks]
    centres = [centres[t] for t in B.track_of_env]
    host = ContactTwin(B, roster, paths, tracks, B.envs_per_track, lib.default_vehicle(), con, pool=pool, M=M, penalty=pen, term_off=term_off,
                       max_steps=max_steps, repeat=R, auto_reset=AR)
    ext, n_tracks = host.ext, len(tracks)
    gen = torch.Generator(device=dev)
    gen.manual_seed(opt.get("seed", 1))
    stream = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)
    keys = ["final_obs", "contact", "final_contact"] + (["state", "final_state"] if state_on else [])

    def reset_both():
        B.reset()
        with torch.cuda.stream(stream):
            o = venv.reset().clone()
            k = venv.contact.clone()
        torch.cuda.synchronize()
        assert not o.cpu().numpy().any() and not k.cpu().numpy().any()
        return o

    obs = reset_both()
    wall_term_of_track = np.zeros(n_tracks, dtype=np.int64)
    wall_streak, term_streak, best_streak = np.zeros(n_envs, dtype=np.int64), np.zeros(n_envs, dtype=np.int64), [0, 0]
    for call in range(calls):
        if call % 60 == 5:                        # bring some cars to the end of their lap: finishes
            teleport(handles, paths, [e for e in range(n_envs) if (e + call) % 5 == 0], ext, cpe)
        if term_off and call % 40 == 27:          # some off the track
            push_off(handles, paths, [e for e in range(n_envs) if (e + call // 40) % 7 == 0], ext, cpe)
        if push in ("walls", "both") and call % 40 == 7:
            push_into_walls(handles, centres, [e for e in range(n_envs) if (e + call // 40) % 6 == 0], ext[:1], cpe)
        if push in ("cars", "both") and call % 40 == 17:
            envs = [e for e in range(n_envs) if (e + call // 40) % 4 == 0]
            nose_to_tail(handles, [e for e in envs if e % 2 == 0], ext[-1], ext[0], cpe)                   # an agent behind an agent
            nose_to_tail(handles, [e for e in envs if e % 2 == 1], ext[-1], 1 if cpe > 2 else ext[0], cpe)  # ... behind the bundled driver's car
        if side and call == calls // 2:
            obs = reset_both()
        with torch.cuda.stream(stream):
            act = torch_driver(torch, obs, gen, dev)
            o, rew, te, tr, info = venv.step(act)
            got = [x.clone() for x in (o, rew, te, tr)] + [info[k].clone() for k in keys]
        torch.cuda.synchronize()
        o, rew, te, tr = [x.cpu().numpy() for x in got[:4]]
        extra = {k: x.cpu().numpy() for k, x in zip(keys, got[4:])}
        obs = got[0]
        want = host.call(act.cpu().numpy().astype(np.float64))
        at = f", call {call}"
        np.testing.assert_array_equal(extra["contact"], want["contact"], err_msg="contact" + at)
        np.testing.assert_array_equal(te, want["terminated"], err_msg="terminated" + at)
        np.testing.assert_array_equal(tr, want["truncated"], err_msg="truncated" + at)
        np.testing.assert_array_equal(rew, want["reward"], err_msg="reward" + at)
        if want["final_obs"] is not None:
            np.testing.assert_array_equal(extra["final_obs"][want["ended"]], want["final_obs"], err_msg="final_obs" + at)
            np.testing.assert_array_equal(extra["final_contact"][want["ended"]], want["final_contact"], err_msg="final_contact" + at)
            if state_on:
                np.testing.assert_array_equal(extra["final_state"][want["ended"]], want["final_state"], err_msg="final_state" + at)
        np.testing.assert_array_equal(o, want["obs"], err_msg="obs" + at)
        if state_on:
            np.testing.assert_array_equal(extra["state"], want["state"], err_msg="state" + at)
        np.add.at(wall_term_of_track, B.track_of_env[want["by_wall"]], 1)
        wall_streak = np.where((want["contact"][:, :, cm.WALL_COUNT] > 0).any(axis=1) | want["by_wall"], wall_streak + 1, 0)
        term_streak = np.where(want["terminated"], term_streak + 1, 0)
        best_streak = [max(best_streak[0], int(wall_streak.max())), max(best_streak[1], int(term_streak.max()))]
    _same_state(A, B)
    c = host.count
    print(f"counts {c}, wall terminations per track {wall_term_of_track.tolist()}, longest wall-contact / terminated run {best_streak}")
    for k in opt.get("need", []):
        assert c[k] > 0, (k, c)
    if opt.get("need_wall_term_per_track"):
        assert (wall_term_of_track > 0).all(), wall_term_of_track
    if not AR:
        np.testing.assert_array_equal(B.steps(), np.full(n_envs, calls * R))
        # nothing is reset: every env has made every step, the penalty was charged call after call, terminated stayed set
        assert best_streak[0] >= 3 and best_streak[1] >= 3 and c["wall_penalised"] > 0 and c["wall_term"] > 0, (best_streak, c)
    print(f"twin ok: {calls} calls, kernel {A.kernel_name()}")
    venv.close()
    B.close()


# ------------------------------------------------------------------------------------------------------------------ off, zero, errors
def _pair(track, kw, x_kw, y_kw):
    from ft_grandprix_amd.vec import DeviceVecEnv
    return DeviceVecEnv(track, **kw, **x_kw), DeviceVecEnv(track, **kw, **y_kw)


def _drive_pair(X, Y, calls, step_x, names, on_call=None):
    """X and Y side by side under the same driver and events; `names` of X equal those of Y at every call."""
    dev = X.device
    track = X.track
    paths, centres = [np.asarray(track.path, dtype=np.float64)] * X.n_envs, [wall_centres(track)] * X.n_envs
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    obs = X.reset().clone()
    Y.reset()
    ends = 0
    for call in range(calls):
        if call % 60 == 5:
            teleport([X.env, Y.env], paths, [e for e in range(X.n_envs) if (e + call) % 5 == 0], [0], 1)
        if call % 40 == 7:
            push_into_walls([X.env, Y.env], centres, [e for e in range(X.n_envs) if (e + call // 40) % 6 == 0], [0], 1)
        act = torch_driver(torch, obs, gen, dev)
        step_x(act)
        Y.step(act)
        torch.cuda.synchronize()
        for name in names:
            np.testing.assert_array_equal(getattr(X, name).cpu().numpy(), getattr(Y, name).cpu().numpy(), err_msg=f"{name}, call {call}")
        if on_call:
            on_call(call)
        ends += int(X.terminated.sum()) + int(X.truncated.sum())
        obs = X.obs.clone()
    _same_state(X.env, Y.env)
    assert ends > 0
    return ends


def off(opt):
    """ftgp_step_device_contacts(io, NULL, NULL) with contacts off against ftgp_step_device on a twin: every output at every call."""
    from ft_grandprix_amd.track import load_track
    kw = dict(n_envs=64, n_rays=120, max_episode_steps=60, lap_target=1, spawn_mode=1, seed=7)
    X, Y = _pair(load_track("small-circle"), kw, {}, {})
    fn = X.env.lib.fn("step_device_contacts")

    def step_x(act):
        X._check_actions(act)
        X._io.action, X._io.stream = act.data_ptr(), torch.cuda.current_stream(X.device).cuda_stream
        X.env.lib.check(fn(X.env.h, X._io_ref, None, None))
    ends = _drive_pair(X, Y, opt.get("calls", 200), step_x, ("obs", "reward", "terminated", "truncated", "final_obs"))
    X.close(); Y.close()
    print(f"off ok: {ends} episode ends")


def zero(opt):
    """A struct of all zeros: the rows are written (the model's, from the twin's read-backs), rewards and episode ends are the twin's."""
    from ft_grandprix_amd.track import load_track
    track = load_track("small-circle")
    kw = dict(n_envs=64, n_rays=120, max_episode_steps=60, lap_target=1, spawn_mode=1, seed=7, auto_reset=False)
    X, Y = _pair(track, kw, dict(contacts=True), {})
    assert X.contacts and X.contact is not None and not Y.contacts and Y.contact is None
    v, seen = X.env.lib.default_vehicle(), [0]

    def on_call(call):
        want = cm.contact_rows(track, v, Y.env.pose(), Y.env.progress()[:, 4], 1, False).reshape(64, 1, 4)       # no reset: the rows of the state as it stands
        np.testing.assert_array_equal(X.contact.cpu().numpy(), want, err_msg=f"contact, call {call}")
        seen[0] += int((want[:, :, 2] > 0).sum())
    ends = _drive_pair(X, Y, opt.get("calls", 200), X.step, ("obs", "reward", "terminated", "truncated"), on_call)
    assert seen[0] > 0
    X.close(); Y.close()
    print(f"zero ok: {ends} episode ends, {seen[0]} rows with a wall contact")


def errors(opt):
    from ft_grandprix_amd import capi
    from ft_grandprix_amd.track import load_track
    from ft_grandprix_amd.vec import DeviceVecEnv
    track = load_track("small-circle")
    lib = capi.load()

    with capi.Env(lib, track, n_envs=8, n_rays=8) as e:
        refused(-4, "contacts before device_io_config", e.device_io_contacts, True)
        refused(-4, "contacts off before device_io_config", e.device_io_contacts, False)
        buf = torch.zeros(8 * 4, device="cuda:0")
        refused(-4, "contacts_device before device_io_config", e.contacts_device, buf.data_ptr())
        assert e.contacts().shape == (8, 4)                        # the read-back works on any handle
    venv = DeviceVecEnv(track, n_envs=8, n_rays=8, max_episode_steps=100, contacts=True, wall_contact_penalty=1.0)
    E = venv.env
    venv.reset()
    act = torch.ones((8, 1, 2), device="cuda:0")
    for _ in range(3):
        venv.step(act)
    torch.cuda.synchronize()

    def snapshot():
        return (E.steps(), E.pose(), E.progress(), E.lidar(), venv.obs.cpu().numpy(), venv.contact.cpu().numpy(), venv.reward.cpu().numpy())
    before = snapshot()
    for what, args in (("a negative wall penalty", (True, False, False, -0.5)), ("a NaN wall penalty", (True, False, False, float("nan"))),
                       ("an infinite wall penalty", (True, False, False, float("inf"))), ("a negative car penalty", (True, False, False, 0.0, -1.0)),
                       ("a NaN car penalty", (True, False, False, 0.0, float("nan"))), ("an infinite car penalty", (True, False, False, 0.0, float("inf")))):
        refused(-1, what, E.device_io_contacts, *args)
    ptrs = [act.data_ptr(), venv.obs.data_ptr(), venv.reward.data_ptr(), venv.terminated.data_ptr(), venv.truncated.data_ptr()]
    host = np.zeros((8, 1, 4), dtype=np.float32)
    refused(-1, "a host pointer for contact", E.step_device, *ptrs, contact=host.ctypes.data)
    refused(-1, "a host pointer for final_contact", E.step_device, *ptrs, contact=venv.contact.data_ptr(), final_contact=host.ctypes.data)
    refused(-1, "a host pointer for ftgp_contacts_device", E.contacts_device, host.ctypes.data)
    torch.cuda.synchronize()
    for x, y in zip(before, snapshot()):          # nothing was enqueued by a refused call, and a refused setter left the rules alone
        np.testing.assert_array_equal(x, y)
    venv.step(act)                                # contacts are still on
    torch.cuda.synchronize()
    np.testing.assert_array_equal(venv.contact.cpu().numpy().reshape(8, 4), E.contacts())
    # ftgp_device_io_signals leaves contacts alone; NULL and a later ftgp_device_io_config turn them off
    E.device_io_signals(1, 0.0)
    venv.step(act)
    torch.cuda.synchronize()
    for turn_off in (lambda: E.device_io_contacts(False), lambda: E.device_io_config(None, 100, 1, True)):
        E.device_io_contacts(True)
        venv.step(act)
        turn_off()
        torch.cuda.synchronize()
        before = snapshot()
        refused(-4, "contact buffers while contacts are off", E.step_device, *ptrs, contact=venv.contact.data_ptr())
        refused(-4, "a final_contact buffer while contacts are off", E.step_device, *ptrs, final_contact=venv.final_contact.data_ptr())
        torch.cuda.synchronize()
        for x, y in zip(before, snapshot()):
            np.testing.assert_array_equal(x, y)
        E.step_device(*ptrs)                      # without contact buffers the call is the old one
        torch.cuda.synchronize()
    venv.close()
    print("errors ok")


SCENARIOS = {"static": static, "twin": twin, "off": off, "zero": zero, "errors": errors}

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
