"""A vectorised environment stepped from torch tensors on the GPU (include/ftgp.h: ftgp_device_io_config / ftgp_step_device).

For drivers that live on the device -- a learned driver, an MLP over the scan, anything written with torch ops -- the host path
(``set_ctrl`` + ``step`` + ``get_lidar``, with a synchronisation each) caps the rate far below what the kernels reach.  Here a step
only enqueues work: the actions are read, the worlds stepped, rewards / episode ends computed and ended envs reset on the device,
ordered on torch's current stream.

One HIP runtime per process.  torch ships its own ``libamdhip64.so``; ``libftgp.so`` resolves its HIP runtime to whichever copy is
already mapped.  Imported after torch, it shares torch's; loaded first, torch then maps a second runtime, and torch's streams and
pointers mean nothing to the library.  This module imports torch before it loads the library, and ``DeviceVecEnv`` refuses to run
in a process that holds two runtimes (``check_single_hip_runtime``).  torch is imported here only; the rest of the package is numpy.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch  # first: the library must bind to torch's HIP runtime (see above)

from . import capi
from .track import Track, load_track

RUNTIME_ERROR = "libftgp.so was loaded before torch in this process; start a fresh process"
ROSTER_NAMES = ("agent", "host", "lobotomy", "nidc", "fast", "random", "net0", "net1", "net2", "net3")


def mapped_hip_runtimes(maps_text: str | None = None) -> dict:
    """{"libamdhip64": [paths], "libhsa-runtime64": [paths]}: the HIP and HSA runtime files mapped into this process."""
    if maps_text is None:
        with open("/proc/self/maps") as f:
            maps_text = f.read()
    out = {"libamdhip64": set(), "libhsa-runtime64": set()}
    for line in maps_text.splitlines():
        parts = line.split(None, 5)
        if len(parts) < 6:
            continue
        path = parts[5].strip()
        base = path.rsplit("/", 1)[-1]
        for name in out:
            if base.startswith(name + ".so"):
                out[name].add(path)
    return {k: sorted(v) for k, v in out.items()}


def check_single_hip_runtime(maps_text: str | None = None) -> None:
    """Raise RuntimeError when more than one HIP or HSA runtime is mapped (libftgp.so was loaded before torch).

    One exception: under rocprofv3 the profiler's own library (librocprofiler-sdk) maps the HSA runtime it was built against beside
    torch's; with a single HIP runtime that second HSA file is the profiler's, not a second runtime of the process's HIP calls."""
    if maps_text is None:
        with open("/proc/self/maps") as f:
            maps_text = f.read()
    rt = mapped_hip_runtimes(maps_text)
    profiler = "librocprofiler-sdk" in maps_text
    for name, paths in rt.items():
        if name == "libhsa-runtime64" and profiler and len(rt["libamdhip64"]) == 1:
            continue
        if len(paths) > 1:
            raise RuntimeError(f"{RUNTIME_ERROR} (two copies of {name} are mapped: {', '.join(paths)})")


class EnvSnapshot:
    """Saved env states (``DeviceVecEnv.save_state``).  ``data``: uint8 [n_rows, bytes_per_env] on the env's device, row e = the
    record of env e (include/ftgp.h: ftgp_save_envs_device; ``capi.unpack_env_state`` decodes it) -- ``data.cpu()`` or ``torch.save``
    of it is the checkpoint.  ``dynamics``: a clone of the env's ``dynamics`` mirror, float64 [n_rows, cars_per_env, 8], None while
    the table is off.  ``generator_state``: the state of the generator the dynamics are drawn with, None without
    ``randomize_dynamics``."""

    def __init__(self, data, dynamics=None, generator_state=None):
        self.data, self.dynamics, self.generator_state = data, dynamics, generator_state

    @property
    def bytes_per_env(self) -> int:
        return int(self.data.shape[1])


class Rollout:
    """T decisions of a network on the device (``DeviceVecEnv.collect``), torch tensors on the env's device with T in front:
    ``inputs`` float32 [T, n_envs, n_agents, n_in] what the network saw, ``mean`` and ``action`` [T, n_envs, n_agents, 2] what it
    proposed and what was applied, ``reward`` [T, n_envs, n_agents], ``terminated`` / ``truncated`` bool [T, n_envs],
    ``next_inputs`` as ``inputs`` (the state after decision t's steps, before any reset; None unless asked for) and ``noise`` the
    draws that were used (None without exploration).  With ``collect(values=True)``: ``value`` and ``next_value`` float32
    [T, n_envs, n_agents], the slot's value net at what ``inputs`` and ``next_inputs`` hold (``next_value`` whether or not
    ``next_inputs`` was recorded), and ``advantage`` / ``returns`` of the advantage scan; None otherwise."""

    def __init__(self, inputs, mean, action, reward, terminated, truncated, next_inputs=None, noise=None, *, value=None, next_value=None,
                 advantage=None, returns=None):
        self.inputs, self.mean, self.action, self.reward = inputs, mean, action, reward
        self.terminated, self.truncated, self.next_inputs, self.noise = terminated, truncated, next_inputs, noise
        self.value, self.next_value, self.advantage, self.returns = value, next_value, advantage, returns


class DeviceVecEnv:
    """``n_envs`` worlds of ``cars_per_env`` cars each, stepped from torch tensors on ``cuda:device_id``.

    roster: one entry per car slot -- "agent" (driven by the caller's actions) or a bundled device driver ("lobotomy", "nidc",
    "fast", "random"); None = every slot an agent.  ``n_agents`` = the number of "agent" slots.

    ``step(actions)`` takes float32 [n_envs, n_agents, 2] = (speed, steering_angle) and returns (obs, reward, terminated,
    truncated, info): obs float32 [n_envs, n_agents, n_rays], reward float32 [n_envs, n_agents] = the change of the car's
    absolute completion, terminated / truncated bool [n_envs], info["final_obs"] = the obs of the envs that ended in the call,
    before their reset (other rows hold older values).

    Signals (include/ftgp.h: ftgp_device_io_signals / ftgp_step_device_ex), all off by default: ``scan_pool`` = rays per beam (a
    divisor of n_rays; obs and final_obs are [n_envs, n_agents, n_beams], n_beams = n_rays / scan_pool, a beam = the nearest hit of
    its rays); ``scan_max_range`` M > 0 clips the ranges to M (no hit = M) and scales them to [0, 1]; ``state=True`` adds
    info["state"] / info["final_state"], float32 [n_envs, n_agents, 8] (capi.STATE_FIELDS), and ``reset()`` fills ``state``;
    ``terminate_off_track`` ends an env when one of its agents is off the track; ``off_track_penalty`` is taken off the reward of an
    agent in every call that leaves it off the track.

    Contacts (ftgp_device_io_contacts / ftgp_step_device_contacts), off by default: ``contacts=True`` adds info["contact"] /
    info["final_contact"], float32 [n_envs, n_agents, 4] (capi.CONTACT_FIELDS: the deepest wall penetration, the deepest overlap with
    an env-mate, the number of the car's contact circles that touch a wall, the number of env-mates it overlaps) at the pose after the
    call's steps; ``terminate_on_wall_contact`` / ``terminate_on_car_contact`` end an env when one of its agents touches a wall / a
    mate, ``wall_contact_penalty`` / ``car_contact_penalty`` are taken off the reward of an agent in every call that leaves it touching.
    Any of the four implies ``contacts=True``; ``reset()`` zeroes ``contact``.

    Track frame (ftgp_device_io_frame / ftgp_step_device_frame), off by default: ``track_frame=True`` adds info["frame"] /
    info["final_frame"], float32 [n_envs, n_agents, 4 + 2 * lookahead]: capi.FRAME_FIELDS -- the signed lateral offset from the
    centre-line (positive = left of the direction of travel), cosine and sine of the track's heading in the car's frame, the continuous
    lap position s / 100 -- then ``lookahead`` (0 .. 16) centre-line points ahead of the car, ``lookahead_stride`` (1 .. 50) path points
    apart, as (forward, left) in the car's frame.  ``frame`` holds the rows after the call, for an env that was reset those of its
    spawn pose; ``final_frame`` the rows before the reset; ``reset()`` fills ``frame``.  ``dense_progress=True`` makes the reward the
    change of s over the call (in path points, a float) in the place of the integer change of absolute completion: zero while the car
    is off the track or has finished; the penalties come off it as before.  ``lookahead`` > 0 or ``dense_progress`` implies
    ``track_frame=True``.

    Rivals (ftgp_device_io_rivals / ftgp_step_device_rivals), off by default: ``rivals=True`` adds info["rival"] / info["final_rival"],
    float32 [n_envs, n_agents, 4 + 8 * n_rivals]: capi.RIVAL_FIELDS -- the car's place in its env's race (1 = in front), the number of
    cars still racing, the gaps in race progress (path points) to the car ahead and to the car behind -- then ``n_rivals`` (0 .. 7)
    mate slots of capi.RIVAL_MATE_FIELDS, nearest unfinished env-mate first: its position, heading and relative velocity in the car's
    frame, the gap along the centre-line, and 1.0; a slot without a mate is zeros, so ``n_rivals`` may exceed ``cars_per_env - 1``.
    ``rival`` holds the rows after the call, for an env that was reset those of its spawn state; ``final_rival`` the rows before the
    reset; ``reset()`` fills ``rival``.  ``place_reward`` w > 0 adds w times the places gained over the call to the reward, behind the
    penalties.  ``n_rivals`` > 0 or ``place_reward`` > 0 implies ``rivals=True``.

    Random starts (ftgp_set_spawn_rule), off by default -- every reset then puts a car back on the pose it had before:
    ``random_start=True`` draws, at every reset of an env (``reset()`` and the auto-reset alike), a start point among the
    ``start_points = (first, count)`` path points (first + i) % 100 that keep ``start_margin`` of wall clearance on both sides (None =
    the chassis' contact radius; with ``bubble_wrap`` the reach of the wheel softeners if that is larger), a lateral offset of up to
    ``start_lateral`` (0 .. 1) of the room the walls leave beyond that margin, a yaw offset of up to ``start_yaw_jitter`` radians to
    either side (``start_yaw_jitter`` < pi), and, with ``shuffle_grid``, the grid slots of the env's cars; keyed by (seed, env,
    episode), so a shard of a larger batch draws what that slice of the whole batch would.  Any of the five implies
    ``random_start=True``.  ``episode_index()`` = how often each env has been reset since.

    Dynamics randomisation (ftgp_set_dynamics_device), off by default -- every car then is the handle's vehicle:
    ``randomize_dynamics`` = a dict from a name of capi.DYN_FIELDS (mass, izz, friction, tire_damping, throttle_kv,
    throttle_force_limit, steer_kp, steer_damping) to ``(lo, hi)`` in absolute units; fields not named keep the handle's value.  A
    fresh row per car is drawn uniformly (a ``torch.Generator`` on the device, seeded with ``dynamics_seed``) at construction and at
    ``reset()`` for every env, and inside every ``step`` for the envs whose episode ended in that call: an env gets new dynamics
    exactly when it starts a new episode, with no host synchronisation.  ``dynamics`` is the torch mirror of the rows in force, float64
    [n_envs, cars_per_env, 8], for privileged critics (None while the table is off).  ``set_dynamics(rows, env_mask=None)`` takes rows
    of the caller's choosing, for curricula.  Not with lidar_mode "fakelidar".

    Network drivers (ftgp_set_net / ftgp_set_net_device): the roster names ``"net0"`` .. ``"net3"`` are slots driven by a frozen MLP
    that the library evaluates inside the step kernel, e.g. ``roster=["agent", "net0", "fast"]``: an earlier policy as an opponent in
    the same world.  ``nets`` = a dict from a slot (0 .. 3) to a ``net.NetSpec`` or an ``nn.Sequential`` with the input fields as
    ``(module, dict(pool=..., max_range=..., beam_first=..., n_beams=...))``; ``set_net(slot, spec_or_module, **input_fields)`` defines
    or replaces one later: the first time, and whenever the shape changes, through the host setter (it synchronises); afterwards, for
    the same shape, through the device setter on torch's current stream.  A roster slot whose network is not defined makes ``step``
    raise.  Action repeat: a network slot is evaluated at every physics step, like the bundled drivers, while an agent's action is
    held for ``action_repeat`` steps -- with ``action_repeat > 1`` a net slot is a different driver from the same network run as an
    agent.  What a net slot sees is what an agent is given with ``scan_pool`` / ``scan_max_range`` / ``state=True`` equal to the
    network's description: the beams ``beam_first .. beam_first + n_beams - 1`` of ``obs`` and entries 0 - 4 of ``state``.
    With frame inputs (``NetSpec(frame=, lookahead=, lookahead_stride=)``, ftgp_set_net_frame) the train-to-deploy rule is: a net slot
    with (``frame``, ``lookahead``, ``lookahead_stride``) sees ``cat(obs[beams], state[:5], frame)`` of an agent whose env has the same
    three settings (``track_frame``, ``lookahead``, ``lookahead_stride``).  The slot's frame inputs do not depend on the env's own
    frame setting: a net slot with frame inputs runs in an env that has the frame off.  ``nets=``, ``set_net`` and ``collect`` follow
    the spec; ``Rollout.inputs`` is as wide as the spec's ``n_in``.
    With rival inputs (``NetSpec(rivals=, n_rivals=)``, ftgp_set_net_rivals) the rule goes one row further: a net slot with ``n_rivals``
    sees ``cat(obs[beams], state[:5], frame, rival)`` of an agent whose env has ``rivals=True`` and the same ``n_rivals`` -- the race
    place, the gaps and the nearest env-mates of the car, every car of the env counted whoever drives it.  The slot's rival inputs are
    its own too: a slot with rival inputs runs in an env whose ``rivals`` is off or has another ``n_rivals``; with one car per env the
    block is (1, 1, 0, 0, zeros).  ``nets=``, ``set_net`` and ``collect`` follow the spec here as well.

    Collected rollouts (ftgp_collect_device): ``collect(n_decisions, slot=0, std=, clip=, noise=, next_inputs=, out=)`` runs T decisions
    of network slot ``slot`` for every agent in one call that only enqueues and returns a ``Rollout`` of torch tensors -- what the
    network saw, its mean, the action applied (mean + std * noise, clipped), the reward and the episode ends per decision -- to the bit
    what T ``step`` calls fed those actions would leave; ``step`` and ``collect`` may alternate.

    Saved states (ftgp_save_envs_device / ftgp_load_envs_device): ``save_state(env_mask=None)`` returns an ``EnvSnapshot`` of the envs'
    whole state -- poses, velocities, steering joint, wheel spins, controls, race and lap fields, step and episode counters, dynamics,
    scans; ``load_state(snap, src=None)`` puts env e back to row ``src[e]`` (negative = keep) and evaluates ``obs`` and the optional
    rows again; ``fork(src)`` = ``load_state(save_state(), src)``, the copy a sampling planner makes.  All on torch's stream.

    The returned tensors are the env's own buffers: the next ``step`` or ``reset`` overwrites them -- clone what you keep.  Work is ordered on ``torch.cuda.current_stream(device)``; nothing
    synchronises the host.

    track: a Track or the name of a bundled track, or a list of them (one handle, ftgp_create_tracks): env block t = envs_per_track[t]
    consecutive envs on track t, as even a split as possible by default.  ``track_index`` (int64 [n_envs], on the env's device) says
    which track each env races, so that a policy can condition on it; ``tracks`` lists the tracks.
    """

    def __init__(self, track, n_envs: int = 4096, n_rays: int = 1080, cars_per_env: int = 1, roster=None,
                 max_episode_steps: int = 3000, action_repeat: int = 1, auto_reset: bool = True, device_id: int = 0,
                 envs_per_track=None, scan_pool: int = 1, scan_max_range: float = 0.0, state: bool = False,
                 terminate_off_track: bool = False, off_track_penalty: float = 0.0, contacts: bool = False,
                 terminate_on_wall_contact: bool = False, terminate_on_car_contact: bool = False, wall_contact_penalty: float = 0.0,
                 car_contact_penalty: float = 0.0, random_start: bool = False, start_points=(0, 100), start_margin=None,
                 start_lateral: float = 0.0, start_yaw_jitter: float = 0.0, shuffle_grid: bool = False, track_frame: bool = False,
                 lookahead: int = 0, lookahead_stride: int = 1, dense_progress: bool = False, rivals: bool = False, n_rivals: int = 0,
                 place_reward: float = 0.0, randomize_dynamics=None, dynamics_seed: int = 0, nets=None, **env_kwargs):
        n_envs, n_rays, cars_per_env = int(n_envs), int(n_rays), int(cars_per_env)
        if n_envs < 1 or n_rays < 1 or not 1 <= cars_per_env <= 8:
            raise ValueError("n_envs >= 1, n_rays >= 1 and 1 <= cars_per_env <= 8")
        if int(action_repeat) < 1:
            raise ValueError("action_repeat >= 1")
        scan_pool, scan_max_range, off_track_penalty = int(scan_pool), float(scan_max_range), float(off_track_penalty)
        if scan_pool < 1 or n_rays % scan_pool:
            raise ValueError(f"scan_pool: >= 1 and a divisor of n_rays = {n_rays}, got {scan_pool}")
        if not (scan_max_range >= 0.0 and math.isfinite(scan_max_range)):
            raise ValueError(f"scan_max_range: >= 0 and finite, got {scan_max_range}")
        if not (off_track_penalty >= 0.0 and math.isfinite(off_track_penalty)):
            raise ValueError(f"off_track_penalty: >= 0 and finite, got {off_track_penalty}")
        wall_contact_penalty, car_contact_penalty = float(wall_contact_penalty), float(car_contact_penalty)
        for name, p in (("wall_contact_penalty", wall_contact_penalty), ("car_contact_penalty", car_contact_penalty)):
            if not (p >= 0.0 and math.isfinite(p)):
                raise ValueError(f"{name}: >= 0 and finite, got {p}")
        try:
            first_point, n_points = (int(v) for v in start_points)
        except (TypeError, ValueError):
            raise ValueError(f"start_points: (first point, number of points), got {start_points!r}") from None
        if not (0 <= first_point < capi.PATH_POINTS and 1 <= n_points <= capi.PATH_POINTS):
            raise ValueError(f"start_points: first point in 0 .. 99 and 1 .. 100 points, got {start_points!r}")
        if start_margin is not None and not (float(start_margin) >= 0.0 and math.isfinite(float(start_margin))):
            raise ValueError(f"start_margin: >= 0 and finite, or None, got {start_margin}")
        start_lateral, start_yaw_jitter = float(start_lateral), float(start_yaw_jitter)
        if not 0.0 <= start_lateral <= 1.0:
            raise ValueError(f"start_lateral: in [0, 1], got {start_lateral}")
        if not 0.0 <= start_yaw_jitter < math.pi:
            raise ValueError(f"start_yaw_jitter: radians in [0, pi), got {start_yaw_jitter}")
        self.random_start = bool(random_start) or (first_point, n_points) != (0, capi.PATH_POINTS) or start_margin is not None or \
            start_lateral > 0.0 or start_yaw_jitter > 0.0 or bool(shuffle_grid)
        lookahead, lookahead_stride = int(lookahead), int(lookahead_stride)
        if not 0 <= lookahead <= capi.MAX_LOOKAHEAD:
            raise ValueError(f"lookahead: 0 .. {capi.MAX_LOOKAHEAD} points, got {lookahead}")
        if not 1 <= lookahead_stride <= capi.PATH_POINTS // 2:
            raise ValueError(f"lookahead_stride: 1 .. {capi.PATH_POINTS // 2} path points, got {lookahead_stride}")
        self.lookahead, self.lookahead_stride, self.dense_progress = lookahead, lookahead_stride, bool(dense_progress)
        self.track_frame = bool(track_frame) or lookahead > 0 or self.dense_progress
        n_rivals, place_reward = int(n_rivals), float(place_reward)
        if not 0 <= n_rivals <= capi.MAX_RIVALS:
            raise ValueError(f"n_rivals: 0 .. {capi.MAX_RIVALS} mate slots, got {n_rivals}")
        if not (place_reward >= 0.0 and math.isfinite(place_reward)):
            raise ValueError(f"place_reward: >= 0 and finite, got {place_reward}")
        self.n_rivals, self.place_reward = n_rivals, place_reward
        self.rivals = bool(rivals) or n_rivals > 0 or place_reward > 0.0
        dyn_bounds = {}
        if randomize_dynamics is not None:
            if not isinstance(randomize_dynamics, dict):
                raise ValueError("randomize_dynamics: a dict from a field of capi.DYN_FIELDS to (lo, hi)")
            for name, bounds in randomize_dynamics.items():
                if name not in capi.DYN_FIELDS:
                    raise ValueError(f"randomize_dynamics: unknown field {name!r}, use one of {capi.DYN_FIELDS}")
                try:
                    lo, hi = (float(b) for b in bounds)
                except (TypeError, ValueError):
                    raise ValueError(f"randomize_dynamics[{name!r}]: (lo, hi), got {bounds!r}") from None
                if not (math.isfinite(lo) and math.isfinite(hi)):
                    raise ValueError(f"randomize_dynamics[{name!r}]: finite bounds, got {bounds!r}")
                if lo > hi:
                    raise ValueError(f"randomize_dynamics[{name!r}]: lo <= hi, got {bounds!r}")
                if (lo <= 0.0) if name in ("mass", "izz") else (lo < 0.0):
                    raise ValueError(f"randomize_dynamics[{name!r}]: lo {'> 0' if name in ('mass', 'izz') else '>= 0'}, got {bounds!r}")
                dyn_bounds[name] = (lo, hi)
        roster = ["agent"] * cars_per_env if roster is None else list(roster)
        if len(roster) != cars_per_env:
            raise ValueError(f"one roster entry per car of an env: expected {cars_per_env}, got {len(roster)}")
        bad = [r for r in roster if r not in ROSTER_NAMES]
        if bad:
            raise ValueError(f"unknown roster entries {bad}: use one of {ROSTER_NAMES}")
        roster = ["agent" if r == "host" else r for r in roster]
        if "agent" not in roster:
            raise ValueError('the roster needs at least one "agent" slot')
        net_specs = {}
        if nets is not None:
            if not isinstance(nets, dict):
                raise ValueError("nets: a dict from a slot (0 .. 3) to a NetSpec, or to (nn.Sequential, dict of input fields)")
            if env_kwargs.get("lidar_mode") in ("fakelidar", capi.LIDAR_FAKELIDAR):
                raise ValueError("network drivers are not available with lidar_mode 'fakelidar'")
            for slot, what in nets.items():
                net_specs[self._check_net_slot(slot)] = self._net_spec(what, n_rays)
        if "lidar_mode" in env_kwargs and env_kwargs["lidar_mode"] not in capi.LIDAR_BY_NAME and env_kwargs["lidar_mode"] not in (0, 1):
            raise ValueError(f"unknown lidar_mode {env_kwargs['lidar_mode']!r}")
        multi = isinstance(track, (list, tuple))
        if not multi and envs_per_track is not None:
            raise ValueError("envs_per_track needs a list of tracks")
        self.tracks = [load_track(t) if isinstance(t, str) else t for t in (track if multi else [track])]
        if not all(isinstance(t, Track) for t in self.tracks):
            raise ValueError("track: a Track or the name of a bundled track, or a list of them")
        self.envs_per_track = capi.track_blocks(n_envs, len(self.tracks), envs_per_track) if multi else (n_envs,)
        self.track = self.tracks[0]
        self.n_envs, self.n_rays, self.cars_per_env, self.roster = n_envs, n_rays, cars_per_env, roster
        self.n_agents = roster.count("agent")
        self.bytes_per_env = capi.env_state_layout(n_rays, cars_per_env)["bytes"]      # of an env-state record (save_state)
        self.max_episode_steps, self.action_repeat, self.auto_reset = int(max_episode_steps), int(action_repeat), bool(auto_reset)
        self.scan_pool, self.scan_max_range, self.n_beams = scan_pool, scan_max_range, n_rays // scan_pool
        self.terminate_off_track, self.off_track_penalty = bool(terminate_off_track), off_track_penalty
        self.terminate_on_wall_contact, self.terminate_on_car_contact = bool(terminate_on_wall_contact), bool(terminate_on_car_contact)
        self.wall_contact_penalty, self.car_contact_penalty = wall_contact_penalty, car_contact_penalty
        self.contacts = bool(contacts) or self.terminate_on_wall_contact or self.terminate_on_car_contact or \
            wall_contact_penalty > 0.0 or car_contact_penalty > 0.0
        signals = scan_pool != 1 or scan_max_range > 0.0 or self.terminate_off_track or off_track_penalty > 0.0

        lib = capi.load()
        check_single_hip_runtime()                   # before any torch GPU call
        self.device = torch.device("cuda", int(device_id))
        if multi:
            env_kwargs["envs_per_track"] = self.envs_per_track
        self.env = capi.Env(lib, self.tracks if multi else self.track, n_envs=n_envs, cars_per_env=cars_per_env, n_rays=n_rays,
                            device_id=int(device_id), **env_kwargs)
        self.env.device_io_config(roster, self.max_episode_steps, self.action_repeat, self.auto_reset)
        if signals:
            self.env.device_io_signals(scan_pool, scan_max_range, self.terminate_off_track, off_track_penalty)
        if self.contacts:
            self.env.device_io_contacts(True, self.terminate_on_wall_contact, self.terminate_on_car_contact, wall_contact_penalty,
                                        car_contact_penalty)
        if self.track_frame:
            self.env.device_io_frame(True, lookahead, lookahead_stride, self.dense_progress)
        if self.rivals:
            self.env.device_io_rivals(True, n_rivals, place_reward)
        self.start_rule = None
        if self.random_start:
            if start_margin is None:       # the chassis circles' radius; with bubble_wrap the softeners' sideways reach if that is larger
                v = self.env.cfg.vehicle
                start_margin = v.contact_radius
                if env_kwargs.get("bubble_wrap"):
                    start_margin = max(start_margin, max(abs(y) for y in v.wheel_y) + v.softener_radius)
            self.start_rule = dict(first_point=first_point, n_points=n_points, margin=float(start_margin), lateral_frac=start_lateral,
                                   yaw_tan=math.tan(0.5 * start_yaw_jitter), shuffle_grid=bool(shuffle_grid))
            self.env.set_spawn_rule(True, **self.start_rule)
        self._nets = {}                              # slot -> (shape key, the device tensor of the parameters last handed over)
        self._pops = {}                              # slot -> (n_members, the device tensors last handed over): slots with a population
        self._vnets = {}                             # slot -> (widths of its value net, the device tensor of the parameters last handed over)
        for slot, spec in net_specs.items():
            self.set_net(slot, spec)
        z = dict(device=self.device)
        self.track_index = torch.from_numpy(self.env.track_of_env.astype("int64")).to(self.device)
        self.obs = torch.zeros((n_envs, self.n_agents, self.n_beams), dtype=torch.float32, **z)
        self.final_obs = torch.zeros_like(self.obs)
        self.reward = torch.zeros((n_envs, self.n_agents), dtype=torch.float32, **z)
        self.terminated = torch.zeros(n_envs, dtype=torch.bool, **z)     # one byte each: the library writes 0 / 1
        self.truncated = torch.zeros(n_envs, dtype=torch.bool, **z)
        self._shape = torch.Size((n_envs, self.n_agents, 2))
        # the call's argument block, built once: a step fills in the action and the stream (the host side of a step is what bounds a
        # one-step call, so it does no more than that)
        self._io = capi.FtgpDeviceStep(None, None, self.obs.data_ptr(), self.reward.data_ptr(), self.terminated.data_ptr(),
                                       self.truncated.data_ptr(), self.final_obs.data_ptr())
        self._io_ref = ctypes.byref(self._io)
        self._step_device = lib.fn("step_device")
        self._step_device_rivals = lib.fn("step_device_rivals")
        # The optional rows, one per agent: name, on?, floats per row (capi.STATE_FIELDS; capi.CONTACT_FIELDS; capi.FRAME_FIELDS, then the
        # look-ahead points; capi.RIVAL_FIELDS, then the mate slots) and the argument struct of ftgp_step_device_rivals that carries the
        # two buffers.  An absent channel leaves
        # its two attributes None and hands the library a null struct.
        channels = (("state", bool(state), capi.STATE_FLOATS, capi.FtgpDeviceStepExtra),
                    ("contact", self.contacts, capi.CONTACT_FLOATS, capi.FtgpDeviceStepContacts),
                    ("frame", self.track_frame, capi.FRAME_FIXED + 2 * lookahead, capi.FtgpDeviceStepFrame),
                    ("rival", self.rivals, capi.RIVAL_FIXED + capi.RIVAL_FLOATS * n_rivals, capi.FtgpDeviceStepRivals))
        self._row_info, self._row_refs = {}, []
        for name, on, width, struct in channels:
            out = torch.zeros((n_envs, self.n_agents, width), dtype=torch.float32, **z) if on else None
            final = torch.zeros_like(out) if on else None
            setattr(self, name, out)
            setattr(self, "final_" + name, final)
            if on:
                self._row_info[name], self._row_info["final_" + name] = out, final
            self._row_refs.append(ctypes.byref(struct(out.data_ptr(), final.data_ptr())) if on else None)
        # dynamics randomisation: the bounds of every field as tensors (a field not named: lo = hi = the handle's value), the generator,
        # the mirror of the rows in force and the mask of a step's draw
        self.dynamics, self._dyn_lo = None, None
        self._set_dynamics_device = lib.fn("set_dynamics_device")
        if randomize_dynamics is not None:
            base = self.env.base_dynamics()
            lo = [dyn_bounds.get(f, (b, b))[0] for f, b in zip(capi.DYN_FIELDS, base)]
            hi = [dyn_bounds.get(f, (b, b))[1] for f, b in zip(capi.DYN_FIELDS, base)]
            self._dyn_lo = torch.tensor(lo, dtype=torch.float64, **z)
            self._dyn_hi = torch.tensor(hi, dtype=torch.float64, **z)
            self._dyn_span = self._dyn_hi - self._dyn_lo
            self._dyn_gen = torch.Generator(device=self.device)
            self._dyn_gen.manual_seed(int(dynamics_seed))
            self._dyn_mask = torch.ones(n_envs, dtype=torch.bool, **z)
            self._dyn_draw = torch.empty((n_envs, cars_per_env, capi.DYN_DOUBLES), dtype=torch.float64, **z)
            self._draw_dynamics(None)

    def _draw_dynamics(self, mask):
        """A fresh table for every car, applied to the envs of ``mask`` (bool [n_envs] on the device, None = all) on torch's stream."""
        with torch.cuda.device(self.device):
            # (five torch launches a draw, into buffers the env keeps: the host side of a step is what bounds a one-step call)
            rows = self._dyn_draw
            rows.uniform_(0.0, 1.0, generator=self._dyn_gen)
            torch.addcmul(self._dyn_lo, self._dyn_span, rows, out=rows)
            torch.minimum(rows, self._dyn_hi, out=rows)
            self._apply_dynamics(rows, mask, valid=True)

    def _apply_dynamics(self, rows, mask, valid=False):
        self._dyn_rows = rows                         # (kept until the next draw: the library reads it in stream order)
        rc = self._set_dynamics_device(self.env.h, torch.cuda.current_stream(self.device).cuda_stream or None, rows.data_ptr(),
                                       None if mask is None else mask.data_ptr())
        if rc:
            self.env.lib.check(rc)
        if self.dynamics is None:
            base = torch.tensor(self.env.base_dynamics(), dtype=torch.float64, device=self.device)
            self.dynamics = base.expand(self.n_envs, self.cars_per_env, capi.DYN_DOUBLES).contiguous()
        if valid:                                    # a draw within checked bounds: every row is taken
            if mask is None:
                self.dynamics.copy_(rows)
            else:
                torch.where(mask[:, None, None], rows, self.dynamics, out=self.dynamics)
            return
        # the library's rule for a row it takes: every entry finite, mass and izz > 0, the others >= 0
        take = (torch.isfinite(rows) & (rows >= 0.0)).all(dim=2) & (rows[:, :, 0] > 0.0) & (rows[:, :, 1] > 0.0)
        if mask is not None:
            take = take & mask.to(torch.bool)[:, None]
        torch.where(take[:, :, None], rows, self.dynamics, out=self.dynamics)

    def set_dynamics(self, rows, env_mask=None):
        """Rows of the caller's choosing (float64 [n_envs, cars_per_env, 8], capi.DYN_FIELDS) for the envs ``env_mask`` (bool or uint8
        [n_envs], None = all) names, on torch's current stream; a car whose row is invalid keeps its old one."""
        rows = torch.as_tensor(rows, dtype=torch.float64, device=self.device).contiguous()
        if rows.shape != (self.n_envs, self.cars_per_env, capi.DYN_DOUBLES):
            raise ValueError(f"rows: shape {(self.n_envs, self.cars_per_env, capi.DYN_DOUBLES)}, got {tuple(rows.shape)}")
        if env_mask is not None:
            env_mask = torch.as_tensor(env_mask, device=self.device)
            if env_mask.shape != (self.n_envs,) or env_mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"env_mask: bool or uint8 [{self.n_envs}], got {env_mask.dtype} {tuple(env_mask.shape)}")
            env_mask = env_mask.contiguous()
        self._dyn_keep = env_mask
        self._apply_dynamics(rows, env_mask)

    @staticmethod
    def _check_net_slot(slot) -> int:
        if isinstance(slot, str) and slot in ROSTER_NAMES[-capi.MAX_NETS:]:
            slot = int(slot[3:])
        if not isinstance(slot, int) or not 0 <= slot < capi.MAX_NETS:
            raise ValueError(f"network slot: 0 .. {capi.MAX_NETS - 1} (or 'net0' .. 'net3'), got {slot!r}")
        return slot

    @staticmethod
    def _net_spec(what, n_rays: int, **input_fields):
        """A NetSpec from a NetSpec, an nn.Sequential (with input fields) or (nn.Sequential, dict), checked against n_rays: everything
        ftgp_set_net checks, without a handle."""
        from . import net
        if isinstance(what, tuple) and len(what) == 2 and isinstance(what[1], dict):
            what, input_fields = what[0], {**what[1], **input_fields}
        if isinstance(what, net.NetSpec):
            if input_fields:
                raise ValueError("a NetSpec carries its input fields")
            spec = what
        else:
            spec = net.from_torch(what, **input_fields)
        spec.check_window(n_rays)
        return spec

    def set_net(self, slot, spec_or_module, **input_fields):
        """Define or replace network slot ``slot`` (0 .. 3 or its roster name).  The first time, and when the shape differs from the
        slot's, through ftgp_set_net (synchronises); for the same shape through ftgp_set_net_device on torch's current stream: the
        self-play loop that refreshes a frozen opponent.  ``None`` clears the slot."""
        slot = self._check_net_slot(slot)
        if spec_or_module is None:
            self.env.set_net(slot, None)
            self._nets.pop(slot, None)
            self._pops.pop(slot, None)
            self._value_nets().pop(slot, None)
            return
        spec = self._net_spec(spec_or_module, self.n_rays, **input_fields)
        key = spec.shape_key()
        if slot in self._nets and self._nets[slot][0] == key and slot not in self._pops:
            with torch.cuda.device(self.device):
                params = torch.from_numpy(spec.flat_params()).to(self.device, non_blocking=False)
                self.env.set_net_device(slot, params.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
            self._nets[slot] = (key, params)         # (kept until the next one: the library reads it in stream order)
            return
        self.env.set_net(slot, spec.layers, **spec.input_fields())      # (defines the slot without a population and without a value net)
        self._nets[slot] = (key, None)
        self._pops.pop(slot, None)
        self._value_nets().pop(slot, None)

    # -- value nets (include/ftgp.h: ftgp_set_value_net)
    def _value_nets(self) -> dict:
        """slot -> (widths of the value net, the device tensor of the parameters last handed over)"""
        if not hasattr(self, "_vnets"):
            self._vnets = {}
        return self._vnets

    def set_value_net(self, slot, spec_or_module, **fields):
        """Give defined slot ``slot`` a value net (a critic over the slot's own input vector): a ``net.ValueSpec`` or an
        ``nn.Sequential`` (``net.value_from_torch``; ``fields``: out_scale, out_offset).  ``None`` clears it.  Synchronises; the
        per-iteration refresh is ``set_value_params``.  ``set_net`` with another shape clears the value net."""
        from . import net
        slot = self._check_net_slot(slot)
        if spec_or_module is None:
            self.env.set_value_net(slot, None)
            self._value_nets().pop(slot, None)
            return
        if slot not in self._nets:
            raise ValueError(f"network slot {slot} is not defined: set_net first")
        spec = spec_or_module if isinstance(spec_or_module, net.ValueSpec) else net.value_from_torch(spec_or_module, **fields)
        if isinstance(spec_or_module, net.ValueSpec) and fields:
            raise TypeError(f"a ValueSpec carries its own fields, got {sorted(fields)} as well")
        n_in = self._nets[slot][0][0][0]
        if spec.n_in != n_in:
            raise ValueError(f"the value net reads slot {slot}'s {n_in} inputs, its first layer has {spec.n_in} columns")
        self.env.set_value_net(slot, spec.layers, **spec.fields())
        self._value_nets()[slot] = (spec.widths, None)

    def set_value_params(self, slot, params):
        """New parameters for a slot's value net from a float32 tensor on the env's device in the flat layout
        (``ValueSpec.flat_params``), on torch's current stream, without a synchronisation: once per learner iteration."""
        slot = self._check_net_slot(slot)
        if slot not in self._value_nets():
            raise ValueError(f"network slot {slot} has no value net: set_value_net first")
        widths = self._vnets[slot][0]
        count = sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.device != self.device or not params.is_contiguous() \
                or tuple(params.shape) != (count,):
            raise ValueError(f"params: a contiguous float32 tensor [{count}] on {self.device}")
        self.env.set_value_net_device(slot, params.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        self._vnets[slot] = (widths, params)           # (kept until the next one: the library reads it in stream order)

    def value_net(self, slot):
        """The slot's value net as the library holds it (synchronises): a ``net.ValueSpec``."""
        from . import net
        slot = self._check_net_slot(slot)
        d, layers = self.env.get_value_net(slot)
        names = {v: k for k, v in capi.ACT_BY_NAME.items()}
        return net.ValueSpec(layers, hidden_act=names[d.hidden_act], out_act=names[d.out_act], out_scale=d.out_scale, out_offset=d.out_offset)

    def gae(self, reward, value, next_value, terminated, truncated, gamma=0.99, lam=0.95, out=None):
        """(advantage, returns) float32 [T, n_envs, n_agents] of the advantage scan (ftgp_gae_device) over tensors shaped as a
        ``Rollout``'s, on torch's current stream; only enqueues.  ``out``: a pair of tensors to write into.  After rescaling the
        rewards of a rollout, ``gae(scaled, r.value, r.next_value, r.terminated, r.truncated, ...)`` gives the advantages again."""
        g, l = capi.check_discounts(gamma, lam)
        if not isinstance(reward, torch.Tensor) or reward.dim() != 3 or tuple(reward.shape[1:]) != (self.n_envs, self.n_agents) or reward.shape[0] < 1:
            raise ValueError(f"reward: a float32 tensor [T, {self.n_envs}, {self.n_agents}] on {self.device}")
        T = int(reward.shape[0])
        lead = (T, self.n_envs, self.n_agents)
        def check(name, t, shape, dtype):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name}: a contiguous {dtype} tensor {shape} on {self.device}")
        for name, t in (("reward", reward), ("value", value), ("next_value", next_value)):
            check(name, t, lead, torch.float32)
        for name, t in (("terminated", terminated), ("truncated", truncated)):
            check(name, t, (T, self.n_envs), torch.bool)
        if out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError("out: a pair (advantage, returns) of tensors")
            check("out[0]", out[0], lead, torch.float32)
            check("out[1]", out[1], lead, torch.float32)
        with self._device_guard():
            adv, ret = out if out is not None else (torch.empty(lead, dtype=torch.float32, device=self.device),
                                                    torch.empty(lead, dtype=torch.float32, device=self.device))
            self._gae_keep = (reward, value, next_value, terminated, truncated, adv, ret)
            self.env.gae_device(T, reward.data_ptr(), value.data_ptr(), next_value.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                                adv.data_ptr(), ret.data_ptr(), gamma=g, lam=l, stream=self._stream())
        return adv, ret

    # -- training on the device (include/ftgp.h: ftgp_train_begin, ftgp_train_grad_device, ftgp_train_adam_device)
    def train_begin(self, slot=0, betas=(0.9, 0.999), eps=1e-8):
        """Give slot ``slot`` (defined, with a value net, without a population) a trainer: zeroed Adam moments and a step count of 0
        (ftgp_train_begin).  ``set_net`` / ``set_value_net`` on the slot end it; ``set_net_params`` / ``set_value_params`` do not."""
        slot = self._check_net_slot(slot)
        d = capi.train_desc(betas, eps)
        if slot not in self._nets:
            raise ValueError(f"network slot {slot} is not defined: set_net first")
        if slot not in self._value_nets():
            raise ValueError(f"network slot {slot} has no value net: set_value_net first")
        if slot in self._pops:
            raise ValueError(f"network slot {slot} carries a population: a trainer steps a single parameter set")
        self.env._call("train_begin", slot, ctypes.byref(d))

    def train_end(self, slot=0):
        self.env.train_end(self._check_net_slot(slot))

    def ppo_update(self, roll, slot=0, epochs=4, minibatches=4, lr=3e-4, clip=0.2, value_coef=0.5, std=(1.0, 1.0), weight=None,
                   normalize_advantage=True, generator=None):
        """Clipped-PPO epochs over a ``collect(values=True)`` rollout on the device: per epoch one ``torch.randperm`` of the rollout's
        rows (int32, on the device, from ``generator``), cut into ``minibatches`` chunks, and per chunk one ftgp_train_grad_device and
        one ftgp_train_adam_device on slot ``slot``'s policy and value net in place (``train_begin`` first).  Only enqueues, on torch's
        current stream; every tensor handed over is kept alive until the next call.  Returns the stats of every chunk, float32
        [epochs * minibatches, 8] on the device (include/ftgp.h: S, policy loss, value loss, approximate KL, clipped fraction, the
        non-finite flag, rows refused, 0).  ``std``: the exploration std the rollout was collected with.  ``weight``: float32
        [T, n_envs, n_agents] >= 0 or None.  ``normalize_advantage``: ONE weighted mean / std over the whole rollout, once per call
        (tools/ppo.py's torch path normalises per minibatch instead)."""
        slot = self._check_net_slot(slot)
        for name, v in (("epochs", epochs), ("minibatches", minibatches)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name}: an integer >= 1, got {v!r}")
        if not isinstance(roll, Rollout) or roll.advantage is None or roll.returns is None:
            raise ValueError("roll: a Rollout of collect(values=True)")
        n_rows = int(roll.advantage.numel())
        if minibatches > n_rows:
            raise ValueError(f"minibatches = {minibatches} exceeds the rollout's {n_rows} rows")
        if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.device != self.device
                                   or tuple(weight.shape) != tuple(roll.advantage.shape) or not weight.is_contiguous()):
            raise ValueError(f"weight: None or a contiguous float32 tensor {tuple(roll.advantage.shape)} on {self.device}")
        probe = capi.train_batch(n_rows, 1, slot=slot, inputs=1, mean=1, advantage=1, ret=1, std=std, clip=clip, value_coef=value_coef)
        with self._device_guard():
            adv = roll.advantage
            if normalize_advantage:
                w = weight if weight is not None else torch.ones_like(adv)
                s = w.sum().clamp_min(1e-12)
                mu = (w * adv).sum() / s
                var = (w * (adv - mu) ** 2).sum() / s
                adv = ((adv - mu) / (var.sqrt() + 1e-8)).contiguous()
            stats = torch.zeros((epochs * minibatches, capi.TRAIN_STATS), dtype=torch.float32, device=self.device)
            stream = self._stream()
            perms = []
            edges = [n_rows * k // minibatches for k in range(minibatches + 1)]
            for ep in range(epochs):
                perm = torch.randperm(n_rows, device=self.device, generator=generator).to(torch.int32)
                perms.append(perm)
                for k in range(minibatches):
                    b = capi.train_batch(n_rows, edges[k + 1] - edges[k], slot=slot, index=perm.data_ptr() + 4 * edges[k],
                                         inputs=roll.inputs.data_ptr(), mean=roll.mean.data_ptr(),
                                         noise=0 if roll.noise is None else roll.noise.data_ptr(), advantage=adv.data_ptr(),
                                         ret=roll.returns.data_ptr(), weight=0 if weight is None else weight.data_ptr(),
                                         std=(probe.std[0], probe.std[1]), clip=probe.clip, value_coef=probe.value_coef,
                                         stats=stats.data_ptr() + 4 * capi.TRAIN_STATS * (ep * minibatches + k), stream=stream)
                    self.env.train_grad_device(b)
                    self.env.train_adam_device(slot, lr, stream)
            self._train_keep = (roll, adv, weight, perms, stats)        # (the library reads and writes them in stream order)
        return stats

    def set_net_params(self, slot, params):
        """New parameters for a defined slot from a float32 tensor on the env's device in ftgp_set_net's flat layout (``NetSpec.flat_params``),
        on torch's current stream, without leaving the device."""
        slot = self._check_net_slot(slot)
        if slot not in self._nets:
            raise ValueError(f"network slot {slot} is not defined: set_net first")
        if slot in self._pops:
            raise ValueError(f"network slot {slot} carries a population: set_population replaces its members")
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.device != self.device or not params.is_contiguous():
            raise ValueError(f"params: a contiguous float32 tensor on {self.device}")
        self.env.set_net_device(slot, params.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        self._nets[slot] = (self._nets[slot][0], params)

    def set_population(self, slot, params, env_member=None):
        """Make defined slot ``slot`` a population (ftgp_set_net_population): ``params`` [n_members, count] float32, a row per member in
        ``NetSpec.flat_params``' layout (``net.stack_params``), and ``env_member`` [n_envs] integers.  ``env_member=None`` is always
        "env e runs member e % n_members"; ``env_member="keep"`` leaves the map of a population of as many members in force (ValueError
        without one).  Env e's cars driven by ``"net<slot>"`` -- in ``step``, ``collect(slot=...)`` and the roster -- then run member
        env_member[e].  numpy arrays go the host way (synchronises; a map entry outside [0, n_members) is a ValueError).  Torch tensors
        on the env's device replace the members and the map (int32) of a population of the same n_members on torch's current stream
        without a synchronisation -- the ES loop --, where a map entry out of range cannot be refused and is taken as member 0; the
        first population of a slot, or another n_members, is allocated through the host way.  ``params=None`` removes the population:
        the slot's own network drives again."""
        slot = self._check_net_slot(slot)
        if slot not in self._nets:
            raise ValueError(f"network slot {slot} is not defined: set_net first")
        if params is None:
            capi.net_population_args(None, None if isinstance(env_member, str) else env_member, self.n_envs)
            self.env.set_net_population(slot, None)
            self._pops.pop(slot, None)
            return
        widths = self._nets[slot][0][0]
        count = sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))
        keep = isinstance(env_member, str)
        if keep:
            n = getattr(params, "shape", (None,))[0]
            if env_member != "keep" or slot not in self._pops or self._pops[slot][0] != n:
                raise ValueError(f'env_member="keep": slot {slot} must carry a population of as many members as params has rows; got {env_member!r}')
        if isinstance(params, torch.Tensor):
            m = None if keep else env_member
            if params.dtype != torch.float32 or params.device != self.device or not params.is_contiguous() or params.dim() != 2:
                raise ValueError(f"params: a contiguous float32 tensor [n_members, count] on {self.device}, or a numpy array")
            if m is not None and (not isinstance(m, torch.Tensor) or m.dtype != torch.int32 or m.device != self.device
                                  or not m.is_contiguous() or tuple(m.shape) != (self.n_envs,)):
                raise ValueError(f"env_member: with a tensor of params, a contiguous int32 tensor [{self.n_envs}] on {self.device}, or None")
            if params.shape[1] != count:
                raise ValueError(f"params: the slot's networks have {count} parameters, got rows of {params.shape[1]}")
            if slot in self._pops and self._pops[slot][0] == params.shape[0]:
                with torch.cuda.device(self.device):
                    if m is None and not keep:
                        m = (torch.arange(self.n_envs, dtype=torch.int32, device=self.device) % params.shape[0]).contiguous()
                    self.env.set_net_population_device(slot, params.data_ptr(), m.data_ptr() if m is not None else 0,
                                                       torch.cuda.current_stream(self.device).cuda_stream)
                self._pops[slot] = (params.shape[0], params, m)      # (kept until the next ones: read in stream order)
                return
            params, env_member = params.cpu().numpy(), (m.cpu().numpy() if m is not None else None)
        if keep:
            env_member = self.env.get_net_population(slot)[1]
        p, m = capi.net_population_args(params, env_member, self.n_envs, count)
        self.env.set_net_population(slot, p, m)
        self._pops[slot] = (p.shape[0], None, None)

    def population(self, slot):
        """(n_members, env_member int32 [n_envs], params float32 [n_members, count]) of a slot's population as the library holds it
        (synchronises), or None for a slot without one."""
        slot = self._check_net_slot(slot)
        n, m = self.env.get_net_population(slot)
        if n == 0:
            return None
        return n, m, np.stack([self.env.get_net_population(slot, k) for k in range(n)])

    def reset(self):
        """Reset every env (synchronous ftgp_reset, which follows the start rule); obs = the scans right after a reset, all zeros
        (custom.py:1092)."""
        self.env.reset()
        if self._dyn_lo is not None:
            self._draw_dynamics(None)
        with torch.cuda.device(self.device):
            self.obs.zero_()
            if self.contact is not None:
                self.contact.zero_()
        if self.state is not None:
            self.env.state_device(self.state.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        if self.frame is not None:
            self.env.frame_device(self.frame.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        if self.rival is not None:
            self.env.rivals_device(self.rival.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return self.obs

    def episode_index(self):
        """int64 numpy [n_envs]: resets of every env since the start rule was set (``Env.episodes``; zeros without random starts)."""
        return self.env.episodes()

    def _check_actions(self, actions):
        if not isinstance(actions, torch.Tensor):
            raise ValueError("actions: a torch tensor")
        if actions.device != self.device:
            raise ValueError(f"actions are on {actions.device}, the env on {self.device}")
        if actions.dtype != torch.float32:
            raise ValueError(f"actions: float32, got {actions.dtype}")
        if actions.shape != self._shape:
            raise ValueError(f"actions: shape {tuple(self._shape)}, got {tuple(actions.shape)}")
        if not actions.is_contiguous():
            raise ValueError("actions: a contiguous tensor")

    def step(self, actions):
        self._check_actions(actions)
        self._io.action = actions.data_ptr()
        self._io.stream = torch.cuda.current_stream(self.device).cuda_stream
        if not self._row_info:
            rc = self._step_device(self.env.h, self._io_ref)      # Env.step_device, without rebuilding the argument block
            if rc:
                self.env.lib.check(rc)
            if self._dyn_lo is not None:
                self._redraw_ended()
            return self.obs, self.reward, self.terminated, self.truncated, {"final_obs": self.final_obs}
        rc = self._step_device_rivals(self.env.h, self._io_ref, *self._row_refs)    # a null struct for an absent channel
        if rc:
            self.env.lib.check(rc)
        if self._dyn_lo is not None:
            self._redraw_ended()
        return self.obs, self.reward, self.terminated, self.truncated, {"final_obs": self.final_obs, **self._row_info}

    def _redraw_ended(self):
        """New dynamics for the envs whose episode ended in the step just enqueued (they start a new episode)."""
        torch.logical_or(self.terminated, self.truncated, out=self._dyn_mask)
        self._draw_dynamics(self._dyn_mask)

    # -- collected rollouts (include/ftgp.h: ftgp_collect_device)
    def collect(self, n_decisions, slot=0, std=(0.0, 0.0), clip=((-1e30, 1e30), (-1e30, 1e30)), noise=None, next_inputs=False, out=None, *,
                values=False, gamma=0.99, lam=0.95):
        """``n_decisions`` = T decisions of network slot ``slot`` for every agent, in one call that only enqueues, on torch's current
        stream: a ``Rollout`` of what the network saw, proposed, what was applied and what came back (ftgp_collect_device).
        action = clip(mean + std * noise) per component, ``clip`` = ((lo, hi) of the speed, (lo, hi) of the steering angle).  ``noise``:
        None = no exploration, True = one ``torch.randn`` on the env's device, or a float32 tensor [T, n_envs, n_agents, 2] of the
        caller's draws.  ``next_inputs=True`` also records the inputs after every decision's steps, before any reset.  ``out``: a
        ``Rollout`` of an earlier call with the same T, slot and ``next_inputs``, whose tensors are written again (with ``noise=True``
        its noise tensor too: drawn into in place).  With
        ``randomize_dynamics`` the T row sets are drawn up front and an env takes decision t's rows when its episode ends there.
        ``obs`` and the optional rows are evaluated again at the state the call leaves, so ``step`` and ``collect`` may alternate.
        ``values=True`` (ftgp_collect_values_device; the slot needs a value net, ``set_value_net``): the ``Rollout`` also holds
        ``value``, ``next_value`` -- the bootstrap of a truncation, with or without ``next_inputs`` -- and ``advantage`` / ``returns`` of
        the advantage scan with ``gamma`` and ``lam``."""
        c = capi.collect_args(n_decisions, slot, std, clip)
        T, slot = c.n_decisions, c.slot
        if slot not in self._nets:
            raise ValueError(f"network slot {slot} is not defined: set_net first")
        v = None
        if values:
            v = capi.collect_values_args(gamma, lam)
            if slot not in self._value_nets():
                raise ValueError(f"network slot {slot} has no value net: set_value_net first")
        n_in = self._nets[slot][0][0][0]
        lead = (T, self.n_envs, self.n_agents)
        if noise is not None and noise is not True:
            if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or noise.device != self.device or \
                    tuple(noise.shape) != lead + (2,) or not noise.is_contiguous():
                raise ValueError(f"noise: None, True or a contiguous float32 tensor {lead + (2,)} on {self.device}")
        shapes = dict(inputs=lead + (n_in,), mean=lead + (2,), action=lead + (2,), reward=lead, terminated=(T, self.n_envs),
                      truncated=(T, self.n_envs))
        if next_inputs:
            shapes["next_inputs"] = lead + (n_in,)
        if values:
            shapes.update(value=lead, next_value=lead, advantage=lead, returns=lead)
        if out is not None:
            if not isinstance(out, Rollout):
                raise ValueError("out: a Rollout of an earlier collect")
            for name, shape in shapes.items():
                t = getattr(out, name)
                want = torch.bool if name in ("terminated", "truncated") else torch.float32
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != want or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"out.{name}: a contiguous {want} tensor {shape} on {self.device} (same T, slot, next_inputs and values)")
        with self._device_guard():
            if out is None:
                out = Rollout(**{name: torch.zeros(shape, dtype=torch.bool if name in ("terminated", "truncated") else torch.float32,
                                                   device=self.device) for name, shape in shapes.items()})
            if not next_inputs:
                out.next_inputs = None
            if not values:
                out.value = out.next_value = out.advantage = out.returns = None
            if noise is True:                            # drawn into the tensor an earlier call left in `out`, if it fits
                kept = out.noise
                fits = isinstance(kept, torch.Tensor) and tuple(kept.shape) == lead + (2,) and kept.dtype == torch.float32 and \
                    kept.device == self.device and kept.is_contiguous()
                noise = kept.normal_() if fits else torch.randn(lead + (2,), dtype=torch.float32, device=self.device)
            out.noise = noise
            rows = None
            if self._dyn_lo is not None:                 # (one block per T, kept on the env and drawn into again)
                shape = (T, self.n_envs, self.cars_per_env, capi.DYN_DOUBLES)
                rows = getattr(self, "_collect_rows", None)
                if rows is None or tuple(rows.shape) != shape:
                    rows = self._collect_rows = torch.empty(shape, dtype=torch.float64, device=self.device)
                rows.uniform_(0.0, 1.0, generator=self._dyn_gen)
                torch.addcmul(self._dyn_lo, self._dyn_span, rows, out=rows)
                torch.minimum(rows, self._dyn_hi, out=rows)
            stream = self._stream()
            for name in ("inputs", "mean", "action", "reward", "terminated", "truncated"):
                setattr(c, name, getattr(out, name).data_ptr())
            c.stream = stream or None
            c.noise = None if noise is None else noise.data_ptr()
            c.next_inputs = out.next_inputs.data_ptr() if next_inputs else None
            c.reset_dynamics = None if rows is None else rows.data_ptr()
            self._collect_keep = (out, noise, rows)      # (the library reads and writes them in stream order)
            if v is not None:
                v.value, v.next_value, v.advantage, v.ret = out.value.data_ptr(), out.next_value.data_ptr(), out.advantage.data_ptr(), out.returns.data_ptr()
                rc = self.env.lib.fn("collect_values_device")(self.env.h, ctypes.byref(c), ctypes.byref(v))
            else:
                rc = self.env.lib.fn("collect_device")(self.env.h, ctypes.byref(c))
            if rc:
                self.env.lib.check(rc)
            if rows is not None:                         # the mirror: the rows of the last decision at which an env ended, if any
                if self.dynamics is None:                # (the table is turned on by the call: every car starts from the handle's values)
                    base = torch.tensor(self.env.base_dynamics(), dtype=torch.float64, device=self.device)
                    self.dynamics = base.expand(self.n_envs, self.cars_per_env, capi.DYN_DOUBLES).contiguous()
                ended = out.terminated | out.truncated
                last = (ended * torch.arange(1, T + 1, device=self.device)[:, None]).amax(dim=0)
                taken = rows[(last - 1).clamp(min=0), torch.arange(self.n_envs, device=self.device)]
                torch.where((last > 0)[:, None, None], taken, self.dynamics, out=self.dynamics)
            self.env.obs_device(self.obs.data_ptr(), stream)
            for buf, refresh in ((self.state, self.env.state_device), (self.contact, self.env.contacts_device),
                                 (self.frame, self.env.frame_device), (self.rival, self.env.rivals_device)):
                if buf is not None:
                    refresh(buf.data_ptr(), stream)
        return out

    # -- env states: save, restore, fork (include/ftgp.h: ftgp_save_envs_device / ftgp_load_envs_device)
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _device_guard(self):
        return torch.cuda.device(self.device)

    def _check_env_vector(self, name, t, dtypes):
        """``t``: a contiguous tensor [n_envs] of one of ``dtypes`` on the env's device (ValueError otherwise)."""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: a torch tensor")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the env on {self.device}")
        if t.dtype not in dtypes:
            raise ValueError(f"{name}: {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if t.shape != (self.n_envs,):
            raise ValueError(f"{name}: shape ({self.n_envs},), got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor")

    def _check_snapshot(self, snap, need_all):
        """``snap``: an EnvSnapshot whose records are this env's, on its device; ``need_all``: with a row for every env."""
        if not isinstance(snap, EnvSnapshot) or not isinstance(snap.data, torch.Tensor):
            raise ValueError("an EnvSnapshot (DeviceVecEnv.save_state)")
        d = snap.data
        if d.dtype != torch.uint8 or d.dim() != 2:
            raise ValueError(f"snapshot data: uint8 [n_rows, bytes_per_env], got {d.dtype} {tuple(d.shape)}")
        if d.shape[1] != self.bytes_per_env:
            raise ValueError(f"snapshot records of {d.shape[1]} bytes, this env's are {self.bytes_per_env} (n_rays {self.n_rays}, "
                             f"{self.cars_per_env} cars per env)")
        if d.device != self.device:
            raise ValueError(f"snapshot data is on {d.device}, the env on {self.device}")
        if not d.is_contiguous() or d.data_ptr() % 16:
            raise ValueError("snapshot data: a contiguous, 16-byte aligned tensor")
        if d.shape[0] < 1 or (need_all and d.shape[0] < self.n_envs):
            raise ValueError(f"snapshot of {d.shape[0]} rows, the env has {self.n_envs} envs")
        if snap.dynamics is not None and (not isinstance(snap.dynamics, torch.Tensor) or snap.dynamics.device != self.device or
                                          snap.dynamics.shape != (d.shape[0], self.cars_per_env, capi.DYN_DOUBLES)):
            raise ValueError(f"snapshot dynamics: float64 [{d.shape[0]}, {self.cars_per_env}, {capi.DYN_DOUBLES}] on {self.device}")

    def save_state(self, env_mask=None, out=None):
        """The state of the envs ``env_mask`` names (bool or uint8 [n_envs] on the device, None = all) as an ``EnvSnapshot``: row e of
        ``data`` is env e's record; a new snapshot holds zeros in the rows of the other envs (no env takes such a row back), ``out`` (a
        snapshot of this env's, with a row per env) keeps what they held.  On torch's current stream; nothing synchronises."""
        if env_mask is not None:
            self._check_env_vector("env_mask", env_mask, (torch.bool, torch.uint8))
        if out is not None:
            self._check_snapshot(out, True)
        with self._device_guard():
            snap = out if out is not None else EnvSnapshot(torch.zeros((self.n_envs, self.bytes_per_env), dtype=torch.uint8,
                                                                       device=self.device))
            self.env.save_envs_device(snap.data.data_ptr(), snap.data.shape[0], 0 if env_mask is None else env_mask.data_ptr(),
                                      self._stream())
            self._state_keep = (snap, env_mask)           # (the library reads and writes them in stream order)
            if self.dynamics is not None:
                if snap.dynamics is None:                      # (a row per record, also beyond the envs in a caller's larger buffer)
                    snap.dynamics = self.dynamics.new_zeros((snap.data.shape[0],) + tuple(self.dynamics.shape[1:]))
                mine = snap.dynamics[:self.n_envs]
                if env_mask is None:
                    mine.copy_(self.dynamics)
                else:
                    torch.where(env_mask.to(torch.bool)[:, None, None], self.dynamics, mine, out=mine)
            snap.generator_state = self._dyn_gen.get_state() if self._dyn_lo is not None else None
        return snap

    def _state_headers(self):
        """uint8 [n_envs, 32] on the device: the header a record must carry for env e to take it (the library's rule)."""
        if getattr(self, "_state_header", None) is None:
            head = np.zeros(self.n_envs, dtype=capi.ENV_STATE_HEADER_DTYPE)
            head["magic"], head["version"] = capi.ENV_STATE_MAGIC, capi.ENV_STATE_VERSION
            head["n_rays"], head["cars_per_env"], head["lidar_mode"] = self.n_rays, self.cars_per_env, self.env.cfg.lidar_mode
            fps = np.array([capi.track_fingerprint(t) for t in self.tracks], dtype=np.uint64)
            head["fingerprint"] = fps[self.env.track_of_env]
            self._state_header = torch.from_numpy(head.view(np.uint8).reshape(self.n_envs, -1)[:, :32].copy()).to(self.device)
        return self._state_header

    def load_state(self, snap, src=None):
        """Put envs back to saved states: env e takes row ``src[e]`` of ``snap`` (int32 or int64 [n_envs] on the device; a negative entry
        keeps the env as it is; None = row e).  A row that is not a record of this env's shape and track, or lies outside the snapshot,
        leaves the env untouched (``env.env_state_rejected()`` counts them).  The ``dynamics`` mirror follows for the envs taken; the
        generator of the dynamics draw is put back only with ``src=None``.  ``obs`` and the ``state`` / ``contact`` / ``frame`` /
        ``rival`` rows are evaluated again at the loaded state; ``reward``, ``terminated``, ``truncated`` and the ``final_*`` buffers
        are left alone.  On torch's current stream; nothing synchronises.  Returns ``obs``."""
        self._check_snapshot(snap, src is None)
        if src is not None:
            self._check_env_vector("src", src, (torch.int32, torch.int64))
        n_rows = snap.data.shape[0]
        with self._device_guard():
            src32 = None if src is None else src.to(torch.int32).contiguous()
            self._state_keep = (snap, src32)
            stream = self._stream()
            self.env.load_envs_device(snap.data.data_ptr(), n_rows, 0 if src32 is None else src32.data_ptr(), stream)
            if self.dynamics is not None and snap.dynamics is not None:
                idx = torch.arange(self.n_envs, device=self.device) if src is None else src.to(torch.int64)
                safe = idx.clamp(0, n_rows - 1)
                take = (idx >= 0) & (idx < n_rows) & (snap.data[safe, :32] == self._state_headers()).all(dim=1)
                torch.where(take[:, None, None], snap.dynamics[safe], self.dynamics, out=self.dynamics)
            if src is None and snap.generator_state is not None and self._dyn_lo is not None:
                self._dyn_gen.set_state(snap.generator_state)
            self.env.obs_device(self.obs.data_ptr(), stream)
            for rows, refresh in ((self.state, self.env.state_device), (self.contact, self.env.contacts_device),
                                  (self.frame, self.env.frame_device), (self.rival, self.env.rivals_device)):
                if rows is not None:
                    refresh(rows.data_ptr(), stream)
        return self.obs

    def fork(self, src):
        """``load_state(save_state(), src)``: env e continues from the state env ``src[e]`` is in now (a negative entry keeps env e).
        What is drawn per env index -- the "random" driver, the next random start -- differs between the copies; everything else
        continues to the bit."""
        self._check_env_vector("src", src, (torch.int32, torch.int64))
        self._fork_snap = self.save_state(out=getattr(self, "_fork_snap", None))      # (one buffer, written whole by every fork)
        return self.load_state(self._fork_snap, src)

    def close(self):
        if getattr(self, "env", None) is not None:
            torch.cuda.current_stream(self.device).synchronize()
            self.env.close()
            self.env = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
