"""ctypes binding of the C-ABI in include/ftgp.h (no PyTorch, numpy buffers only).

``load()`` opens the HIP library built by ``__graft_entry__.build()`` and fails loudly
when it is missing -- the product has no CPU fallback.  ``CLib`` is generic over the
symbol prefix so that the test-suite can bind the CPU oracle (same signatures, prefix
``oracle_``) through the same wrapper; nothing in this package loads the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .track import Track

ABI_VERSION = 5
PATH_POINTS = 100
MAX_LAP_TIMES = 32
SNAPSHOT_DOUBLES = 10
POSE_DOUBLES = 13
PROGRESS_INTS = 10
METRIC_DOUBLES = 8
STATE_FLOATS = 8            # FTGP_STATE_FLOATS: a state row of the device step (STATE_FIELDS)
CONTACT_FLOATS = 4          # FTGP_CONTACT_FLOATS: a contact row (CONTACT_FIELDS)
FRAME_FIXED = 4              # FTGP_FRAME_FIXED: the fixed entries of a frame row (FRAME_FIELDS); 2 floats per look-ahead point follow
MAX_LOOKAHEAD = 16           # FTGP_MAX_LOOKAHEAD
RIVAL_FIXED = 4              # FTGP_RIVAL_FIXED: the fixed entries of a rival row (RIVAL_FIELDS); RIVAL_FLOATS floats per mate slot follow
RIVAL_FLOATS = 8             # FTGP_RIVAL_FLOATS: a mate slot (RIVAL_MATE_FIELDS)
MAX_RIVALS = 7               # FTGP_MAX_RIVALS
MAX_TRACKS = 16             # FTGP_MAX_TRACKS: tracks of one multi-track handle (ftgp_create_tracks)
DYN_DOUBLES = 8             # FTGP_DYN_DOUBLES: a dynamics row of a car (DYN_FIELDS; ftgp_set_dynamics)
DYN_RECORD = 12             # FTGP_DYN_RECORD: a dynamics record of an env-state record: the row, then the four static wheel loads
ENV_STATE_VERSION = 1       # FTGP_ENV_STATE_VERSION
ENV_STATE_MAGIC = 0x53454746    # FTGP_ENV_STATE_MAGIC

POLICY_HOST, POLICY_LOBOTOMY, POLICY_NIDC, POLICY_FAST, POLICY_RANDOM = 0, 1, 2, 3, 4
LIDAR_RANGEFINDER, LIDAR_FAKELIDAR = 0, 1
LIDAR_BY_NAME = {"rangefinder": LIDAR_RANGEFINDER, "fakelidar": LIDAR_FAKELIDAR}
POLICY_PER_CAR = 5
POLICY_NET0 = 6             # FTGP_POLICY_NET0 .. FTGP_POLICY_NET3: the network drivers of slots 0 .. 3 (ftgp_set_net)
MAX_NETS = 4                # FTGP_MAX_NETS
NET_MAX_LAYERS, NET_MAX_INPUTS, NET_MAX_HIDDEN, NET_STATE_INPUTS = 4, 256, 128, 5       # FTGP_NET_*
ACT_IDENTITY, ACT_RELU, ACT_TANH = 0, 1, 2
ACT_BY_NAME = {"identity": ACT_IDENTITY, "relu": ACT_RELU, "tanh": ACT_TANH}
POLICY_BY_NAME = {"host": POLICY_HOST, "lobotomy": POLICY_LOBOTOMY, "nidc": POLICY_NIDC,
                  "fast": POLICY_FAST, "random": POLICY_RANDOM, "per_car": POLICY_PER_CAR,
                  "net0": POLICY_NET0, "net1": POLICY_NET0 + 1, "net2": POLICY_NET0 + 2, "net3": POLICY_NET0 + 3}

PROGRESS_FIELDS = ("laps", "completion", "lap_completion", "absolute_completion", "finished",
                   "off_track", "start", "good_start", "delta", "finish_step")
STATE_FIELDS = ("v_long", "v_lat", "wz", "u_speed", "u_steer", "centre_dist", "lap_completion", "off_track")
CONTACT_FIELDS = ("wall_pen", "car_pen", "wall_count", "car_count")
FRAME_FIELDS = ("lat", "cos_h", "sin_h", "s_norm")
RIVAL_FIELDS = ("place", "n_racing", "gap_ahead", "gap_behind")
RIVAL_MATE_FIELDS = ("fwd", "left", "cos_rel", "sin_rel", "v_fwd", "v_left", "track_gap", "present")
DYN_FIELDS = ("mass", "izz", "friction", "tire_damping", "throttle_kv", "throttle_force_limit", "steer_kp", "steer_damping")
METRIC_FIELDS = ("steps", "n_cars", "sum_laps", "sum_absolute_completion", "n_finished",
                 "n_off_track", "min_lap_time", "max_lap_time")


class FtgpTrack(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("words_per_row", C.c_int32),
                ("reserved0", C.c_int32), ("bits", C.c_void_p),
                ("px_size_x", C.c_double), ("px_size_y", C.c_double),
                ("origin_x", C.c_double), ("origin_y", C.c_double), ("path", C.c_void_p)]


class FtgpVehicle(C.Structure):
    _fields_ = [("mass", C.c_double), ("izz", C.c_double),
                ("wheel_x", C.c_double * 4), ("wheel_y", C.c_double * 4),
                ("wheel_radius", C.c_double), ("wheel_inertia", C.c_double), ("wheel_damping", C.c_double),
                ("throttle_kv", C.c_double), ("throttle_gear", C.c_double), ("throttle_force_limit", C.c_double),
                ("steer_kp", C.c_double), ("steer_damping", C.c_double), ("steer_inertia", C.c_double),
                ("steer_limit", C.c_double),
                ("friction", C.c_double), ("gravity", C.c_double), ("tire_damping", C.c_double),
                ("contact_x", C.c_double * 3), ("contact_radius", C.c_double),
                ("contact_stiffness", C.c_double), ("contact_damping", C.c_double),
                ("lidar_x", C.c_double), ("lidar_y", C.c_double), ("lidar_ring_radius", C.c_double),
                ("body_z", C.c_double),
                ("box_xmin", C.c_double), ("box_xmax", C.c_double), ("box_ymin", C.c_double), ("box_ymax", C.c_double),
                ("softener_radius", C.c_double), ("motor_forward_limit", C.c_double), ("motor_turn_limit", C.c_double),
                ("kind", C.c_int32), ("reserved1", C.c_int32)]


class FtgpConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_envs", C.c_int32), ("cars_per_env", C.c_int32),
                ("n_rays", C.c_int32), ("lap_target", C.c_int32), ("device_id", C.c_int32),
                ("spawn_mode", C.c_int32), ("env_base", C.c_int32), ("seed", C.c_uint64),
                ("dt", C.c_double), ("bubble_wrap", C.c_int32), ("naive_flatten", C.c_int32),
                ("lidar_mode", C.c_int32), ("reserved2", C.c_int32), ("map_size", C.c_double), ("fan_dirs", C.c_void_p),
                ("track", FtgpTrack), ("vehicle", FtgpVehicle)]


# every symbol include/ftgp.h declares (checked by tests/test_capi.py)
API_SYMBOLS = (
    "default_vehicle", "tricycle_vehicle", "last_error", "device_count", "create", "destroy", "reset", "set_ctrl", "step",
    "rollout", "set_car_policies", "get_lidar", "get_snapshot", "get_pose", "get_progress", "get_winners", "get_lap_times", "get_ctrl",
    "get_steps", "set_pose", "policy_eval", "eval_progress", "metrics_local", "comm_unique_id", "comm_init", "metrics_allgather",
    "metrics_allgather_begin", "metrics_allgather_end", "get_distance_field",
    "last_kernel_ms", "kernel_name", "fakelidar", "selftest", "build_info", "get_race_steps",
    "device_io_config", "step_device", "create_tracks", "get_track_distance_field",
    "device_io_signals", "step_device_ex", "state_device", "get_centre_dist2",
    "device_io_contacts", "step_device_contacts", "contacts_device", "get_contacts",
    "set_spawn_rule", "get_episodes", "get_start_table",
    "device_io_frame", "step_device_frame", "frame_device", "get_frames",
    "device_io_rivals", "step_device_rivals", "rivals_device", "get_rivals",
    "set_dynamics", "set_dynamics_device", "get_dynamics",
    "env_state_bytes", "save_envs_device", "load_envs_device", "get_env_state_rejected", "obs_device",
    "set_net", "set_net_device", "get_net", "set_net_frame", "get_net_frame", "set_net_rivals", "get_net_rivals",
    "collect_device",
    "set_net_population", "set_net_population_device", "get_net_population",
    "set_value_net", "set_value_net_device", "get_value_net", "collect_values_device", "gae_device",
    "train_begin", "train_end", "train_grad_device", "train_adam_device", "train_get",
)


class FtgpDeviceIoConfig(C.Structure):
    _fields_ = [("roster", C.c_void_p), ("max_episode_steps", C.c_int64), ("action_repeat", C.c_int32), ("auto_reset", C.c_int32)]


class FtgpDeviceStep(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("action", C.c_void_p), ("obs", C.c_void_p), ("reward", C.c_void_p),
                ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("final_obs", C.c_void_p)]


class FtgpDeviceSignals(C.Structure):
    _fields_ = [("scan_pool", C.c_int32), ("scan_max_range", C.c_float), ("terminate_off_track", C.c_int32),
                ("off_track_penalty", C.c_float)]


class FtgpDeviceStepExtra(C.Structure):
    _fields_ = [("state", C.c_void_p), ("final_state", C.c_void_p)]


class FtgpDeviceContacts(C.Structure):
    _fields_ = [("terminate_on_wall", C.c_int32), ("terminate_on_car", C.c_int32), ("wall_penalty", C.c_float),
                ("car_penalty", C.c_float)]


class FtgpDeviceStepContacts(C.Structure):
    _fields_ = [("contact", C.c_void_p), ("final_contact", C.c_void_p)]


class FtgpDeviceFrame(C.Structure):
    _fields_ = [("n_ahead", C.c_int32), ("stride", C.c_int32), ("dense_progress", C.c_int32), ("reserved", C.c_int32)]


class FtgpDeviceStepFrame(C.Structure):
    _fields_ = [("frame", C.c_void_p), ("final_frame", C.c_void_p)]


class FtgpDeviceRivals(C.Structure):
    _fields_ = [("n_rivals", C.c_int32), ("reserved", C.c_int32), ("place_weight", C.c_float), ("reserved_f", C.c_float)]


class FtgpDeviceStepRivals(C.Structure):
    _fields_ = [("rival", C.c_void_p), ("final_rival", C.c_void_p)]


class FtgpSpawnRule(C.Structure):
    _fields_ = [("first_point", C.c_int32), ("n_points", C.c_int32), ("shuffle_grid", C.c_int32), ("reserved", C.c_int32),
                ("margin", C.c_double), ("lateral_frac", C.c_double), ("yaw_tan", C.c_double)]


class FtgpNetDesc(C.Structure):
    _fields_ = [("pool", C.c_int32), ("max_range", C.c_float), ("beam_first", C.c_int32), ("n_beams", C.c_int32),
                ("use_state", C.c_int32), ("n_layers", C.c_int32), ("width", C.c_int32 * NET_MAX_LAYERS),
                ("hidden_act", C.c_int32), ("out_act", C.c_int32), ("out_scale", C.c_float * 2), ("out_offset", C.c_float * 2),
                ("reserved", C.c_int32)]


class FtgpNetFrame(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("n_ahead", C.c_int32), ("stride", C.c_int32), ("reserved", C.c_int32)]


class FtgpNetRivals(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("n_rivals", C.c_int32), ("reserved", C.c_int32 * 2)]


class FtgpCollect(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("slot", C.c_int32), ("n_decisions", C.c_int32), ("std", C.c_float * 2), ("lo", C.c_float * 2),
                ("hi", C.c_float * 2), ("noise", C.c_void_p), ("inputs", C.c_void_p), ("mean", C.c_void_p), ("action", C.c_void_p),
                ("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p), ("next_inputs", C.c_void_p),
                ("reset_dynamics", C.c_void_p), ("reserved", C.c_int32)]


def collect_args(n_decisions, slot=0, std=(0.0, 0.0), clip=((-1e30, 1e30), (-1e30, 1e30))) -> "FtgpCollect":
    """An FtgpCollect with the scalar fields set and every check of ftgp_collect_device that needs no handle (ValueError): T >= 1, a
    slot in 0 .. 3, std >= 0 and finite, a finite clip with lo <= hi per component.  The buffers are left NULL."""
    if isinstance(n_decisions, bool) or not isinstance(n_decisions, (int, np.integer)) or not 1 <= int(n_decisions) < 2 ** 31:
        raise ValueError(f"n_decisions: an integer >= 1, got {n_decisions!r}")
    if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < MAX_NETS:
        raise ValueError(f"network slot: 0 .. {MAX_NETS - 1}, got {slot!r}")
    try:
        sd = np.asarray(std, dtype=np.float32)
        lim = np.asarray(clip, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"std: two numbers, clip: ((lo, hi), (lo, hi)); got {std!r}, {clip!r}") from None
    if sd.shape != (2,) or not (np.isfinite(sd).all() and (sd >= 0).all()):
        raise ValueError(f"std: two finite numbers >= 0 (speed, steering_angle), got {std!r}")
    if lim.shape != (2, 2) or not np.isfinite(lim).all() or not (lim[:, 0] <= lim[:, 1]).all():
        raise ValueError(f"clip: ((lo, hi), (lo, hi)), finite with lo <= hi, got {clip!r}")
    c = FtgpCollect(slot=int(slot), n_decisions=int(n_decisions))
    for k in range(2):
        c.std[k], c.lo[k], c.hi[k] = float(sd[k]), float(lim[k, 0]), float(lim[k, 1])
    return c


class FtgpValueDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("width", C.c_int32 * NET_MAX_LAYERS), ("hidden_act", C.c_int32), ("out_act", C.c_int32),
                ("out_scale", C.c_float), ("out_offset", C.c_float), ("reserved", C.c_int32)]


class FtgpCollectValues(C.Structure):
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("value", C.c_void_p), ("next_value", C.c_void_p),
                ("advantage", C.c_void_p), ("ret", C.c_void_p), ("reserved", C.c_int32 * 2)]


def value_desc(layers, *, hidden_act="tanh", out_act="identity", out_scale=1.0, out_offset=0.0):
    """(FtgpValueDesc, flat float32 parameters) of a value net given as a list of (W [n_out, n_in], b [n_out]) pairs, with every check
    of ftgp_set_value_net that needs no handle (ValueError): 1 .. 4 layers, hidden widths 1 .. 128, a last width of exactly 1, the
    activations, a finite output map, the shapes of the arrays.  The first layer's n_in must be the slot's; the handle knows it."""
    try:
        layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
    except (TypeError, ValueError):
        raise ValueError("layers: a list of (W [n_out, n_in], b [n_out]) pairs") from None
    if not 1 <= len(layers) <= NET_MAX_LAYERS:
        raise ValueError(f"a value net has 1 .. {NET_MAX_LAYERS} layers, got {len(layers)}")
    for name, act in (("hidden_act", hidden_act), ("out_act", out_act)):
        if act not in ACT_BY_NAME:
            raise ValueError(f"{name}: one of {sorted(ACT_BY_NAME)}, got {act!r}")
    try:
        scale, offset = float(np.float32(out_scale)), float(np.float32(out_offset))
    except (TypeError, ValueError):
        raise ValueError(f"out_scale and out_offset: one finite number each, got {out_scale!r}, {out_offset!r}") from None
    if not (np.isfinite(scale) and np.isfinite(offset)):
        raise ValueError(f"out_scale and out_offset: one finite number each, got {out_scale!r}, {out_offset!r}")
    d = FtgpValueDesc(n_layers=len(layers), hidden_act=ACT_BY_NAME[hidden_act], out_act=ACT_BY_NAME[out_act], out_scale=scale, out_offset=offset)
    flat, width = [], None
    for l, (W, b) in enumerate(layers):
        last = l == len(layers) - 1
        if W.ndim != 2 or W.shape[1] < 1 or (width is not None and W.shape[1] != width) or b.shape != (W.shape[0],):
            raise ValueError(f"layer {l}: W [n_out, {width if width is not None else 'n_in'}] and b [n_out] (torch's nn.Linear layout), got {W.shape} and {b.shape}")
        if last and W.shape[0] != 1:
            raise ValueError(f"the last layer of a value net has exactly 1 output, got {W.shape[0]}")
        if not last and not 1 <= W.shape[0] <= NET_MAX_HIDDEN:
            raise ValueError(f"layer {l}: a hidden width is 1 .. {NET_MAX_HIDDEN}, got {W.shape[0]}")
        d.width[l] = width = W.shape[0]
        flat += [W.ravel(), b.ravel()]
    if layers[0][0].shape[1] > NET_MAX_INPUTS:
        raise ValueError(f"layer 0: at most {NET_MAX_INPUTS} inputs, got {layers[0][0].shape[1]}")
    return d, np.ascontiguousarray(np.concatenate(flat), dtype=np.float32)


def value_param_count(d: FtgpValueDesc, n_in: int) -> int:
    n = 0
    for l in range(d.n_layers):
        n, n_in = n + d.width[l] * n_in + d.width[l], d.width[l]
    return n


def value_layers(d: FtgpValueDesc, flat: np.ndarray, n_in: int) -> list:
    """The (W, b) pairs of a value net's flat parameter buffer on a slot of ``n_in`` inputs."""
    out, o = [], 0
    for l in range(d.n_layers):
        n_out = d.width[l]
        W = flat[o:o + n_out * n_in].reshape(n_out, n_in); o += n_out * n_in
        out.append((W.copy(), flat[o:o + n_out].copy())); o += n_out
        n_in = n_out
    return out


def check_discounts(gamma, lam):
    """gamma and lam of ftgp_collect_values_device and ftgp_gae_device as binary32 (ValueError): finite, in [0, 1]."""
    out = []
    for name, v in (("gamma", gamma), ("lam", lam)):
        try:
            f = float(np.float32(v))
        except (TypeError, ValueError):
            raise ValueError(f"{name}: a number in [0, 1], got {v!r}") from None
        if isinstance(v, bool) or not (np.isfinite(f) and 0.0 <= f <= 1.0):
            raise ValueError(f"{name}: finite and in [0, 1], got {v!r}")
        out.append(f)
    return tuple(out)


def collect_values_args(gamma=0.99, lam=0.95, value: int = 0, next_value: int = 0, advantage: int = 0, ret: int = 0) -> "FtgpCollectValues":
    """An FtgpCollectValues on integer device addresses with every check of ftgp_collect_values_device that needs no handle
    (ValueError): gamma and lam finite and in [0, 1]; ``advantage`` and ``ret`` both or neither (0 = NULL)."""
    g, l = check_discounts(gamma, lam)
    if bool(advantage) != bool(ret):
        raise ValueError("advantage and ret: both or neither" + (", got advantage without ret" if advantage else ", got ret without advantage"))
    v = FtgpCollectValues(gamma=g, lam=l)
    for name, a in (("value", value), ("next_value", next_value), ("advantage", advantage), ("ret", ret)):
        setattr(v, name, a or None)
    return v


TRAIN_STATS = 8
TRAIN_GRAD, TRAIN_M, TRAIN_V, TRAIN_RAW_GRAD, TRAIN_RAW_PARAMS = 0, 1, 2, 3, 4


class FtgpTrainDesc(C.Structure):
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("reserved", C.c_int32)]


class FtgpTrainBatch(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("slot", C.c_int32), ("n_rows", C.c_int32), ("n_batch", C.c_int32), ("first_row", C.c_int32),
                ("index", C.c_void_p), ("inputs", C.c_void_p), ("mean", C.c_void_p), ("noise", C.c_void_p), ("advantage", C.c_void_p),
                ("ret", C.c_void_p), ("weight", C.c_void_p), ("std", C.c_float * 2), ("clip", C.c_float), ("value_coef", C.c_float),
                ("stats", C.c_void_p), ("new_mean", C.c_void_p), ("new_value", C.c_void_p), ("reserved", C.c_int32 * 2)]


def _f32(name, v, what, ok):
    try:
        f = float(np.float32(v))
    except (TypeError, ValueError):
        raise ValueError(f"{name}: {what}, got {v!r}") from None
    if isinstance(v, bool) or not (np.isfinite(f) and ok(f)):
        raise ValueError(f"{name}: {what}, got {v!r}")
    return f


def _train_slot(slot):
    if isinstance(slot, bool) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < MAX_NETS:
        raise ValueError(f"network slot: 0 .. {MAX_NETS - 1}, got {slot!r}")
    return int(slot)


def train_desc(betas=(0.9, 0.999), eps=1e-8) -> "FtgpTrainDesc":
    """The FtgpTrainDesc of ftgp_train_begin with its checks (ValueError): two betas, finite and in [0, 1); eps finite and > 0."""
    try:
        b1, b2 = betas
    except (TypeError, ValueError):
        raise ValueError(f"betas: two numbers in [0, 1), got {betas!r}") from None
    return FtgpTrainDesc(beta1=_f32("beta1", b1, "finite and in [0, 1)", lambda f: 0.0 <= f < 1.0),
                         beta2=_f32("beta2", b2, "finite and in [0, 1)", lambda f: 0.0 <= f < 1.0),
                         eps=_f32("eps", eps, "finite and > 0", lambda f: f > 0.0))


def train_batch(n_rows, n_batch, *, slot=0, first_row=0, index: int = 0, inputs: int = 0, mean: int = 0, noise: int = 0, advantage: int = 0,
                ret: int = 0, weight: int = 0, std=(1.0, 1.0), clip=0.2, value_coef=0.5, stats: int = 0, new_mean: int = 0, new_value: int = 0,
                stream: int = 0) -> "FtgpTrainBatch":
    """An FtgpTrainBatch on integer device addresses (0 = NULL) with every check of ftgp_train_grad_device that needs no handle
    (ValueError): n_rows and n_batch >= 1, the range of first_row (without an index), std finite and > 0, clip and value_coef finite and
    >= 0, the required buffers given."""
    for name, v in (("n_rows", n_rows), ("n_batch", n_batch)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) < 2 ** 31:
            raise ValueError(f"{name}: an integer >= 1, got {v!r}")
    if isinstance(first_row, bool) or not isinstance(first_row, (int, np.integer)):
        raise ValueError(f"first_row: an integer, got {first_row!r}")
    if not index and not 0 <= int(first_row) <= int(n_rows) - int(n_batch):
        raise ValueError(f"first_row = {first_row} with n_batch = {n_batch} leaves the {n_rows} rows")
    try:
        s0, s1 = std
    except (TypeError, ValueError):
        raise ValueError(f"std: two finite numbers > 0, got {std!r}") from None
    b = FtgpTrainBatch(slot=_train_slot(slot), n_rows=int(n_rows), n_batch=int(n_batch), first_row=int(first_row) if not index else 0,
                       clip=_f32("clip", clip, "finite and >= 0", lambda f: f >= 0.0),
                       value_coef=_f32("value_coef", value_coef, "finite and >= 0", lambda f: f >= 0.0))
    b.std[0] = _f32("std[0]", s0, "finite and > 0", lambda f: f > 0.0)
    b.std[1] = _f32("std[1]", s1, "finite and > 0", lambda f: f > 0.0)
    for name, a in (("inputs", inputs), ("mean", mean), ("advantage", advantage), ("ret", ret)):
        if not a:
            raise ValueError(f"{name}: a device address, got {a!r}")
    for name, a in (("stream", stream), ("index", index), ("inputs", inputs), ("mean", mean), ("noise", noise), ("advantage", advantage),
                    ("ret", ret), ("weight", weight), ("stats", stats), ("new_mean", new_mean), ("new_value", new_value)):
        setattr(b, name, a or None)
    return b


def net_frame(frame=False, lookahead=0, lookahead_stride=1) -> "FtgpNetFrame":
    """The FtgpNetFrame of ftgp_set_net_frame with its checks (ValueError): lookahead 0 .. 16 and lookahead_stride 1 .. 50, checked
    with the frame off too; ``lookahead > 0`` implies ``frame``, as in DeviceVecEnv."""
    for name, v, lo, hi in (("lookahead", lookahead, 0, MAX_LOOKAHEAD), ("lookahead_stride", lookahead_stride, 1, 50)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name}: an integer in {lo} .. {hi}, got {v!r}")
    return FtgpNetFrame(enabled=1 if (frame or int(lookahead) > 0) else 0, n_ahead=int(lookahead), stride=int(lookahead_stride))


def net_frame_inputs(f) -> int:
    """Frame entries behind the beams and the state inputs: 0 without frame inputs (``f`` an FtgpNetFrame or None)."""
    return FRAME_FIXED + 2 * f.n_ahead if f is not None and f.enabled else 0


def net_rivals(rivals=False, n_rivals=0) -> "FtgpNetRivals":
    """The FtgpNetRivals of ftgp_set_net_rivals with its checks (ValueError): n_rivals 0 .. 7, checked with rivals off too;
    ``n_rivals > 0`` implies ``rivals``, as ``lookahead`` does for ``frame``."""
    if isinstance(n_rivals, bool) or not isinstance(n_rivals, (int, np.integer)) or not 0 <= int(n_rivals) <= MAX_RIVALS:
        raise ValueError(f"n_rivals: an integer in 0 .. {MAX_RIVALS}, got {n_rivals!r}")
    return FtgpNetRivals(enabled=1 if (rivals or int(n_rivals) > 0) else 0, n_rivals=int(n_rivals))


def net_rival_inputs(r) -> int:
    """Rival entries at the end of the input vector: 0 without rival inputs (``r`` an FtgpNetRivals or None)."""
    return RIVAL_FIXED + RIVAL_FLOATS * r.n_rivals if r is not None and r.enabled else 0


def net_desc(layers, *, pool, max_range, beam_first, n_beams, use_state=False, hidden_act="tanh", out_act="tanh",
             out_scale=(1, 1), out_offset=(0, 0), frame=False, lookahead=0, lookahead_stride=1, rivals=False, n_rivals=0):
    """(FtgpNetDesc, flat float32 parameters) of a network given as a list of (W [n_out, n_in], b [n_out]) pairs, with every check of
    ftgp_set_net and ftgp_set_net_frame that needs no handle (ValueError): the widths, the activations, the output map, the shapes of
    the arrays, the frame fields (``net_frame`` makes the struct) and the rival fields (``net_rivals``).  The window rule needs n_rays:
    ``check_net_window``."""
    n_frame = net_frame_inputs(net_frame(frame, lookahead, lookahead_stride))
    n_rival = net_rival_inputs(net_rivals(rivals, n_rivals))
    layers = [(np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)) for W, b in layers]
    if not 1 <= len(layers) <= NET_MAX_LAYERS:
        raise ValueError(f"a network has 1 .. {NET_MAX_LAYERS} layers, got {len(layers)}")
    if int(pool) < 1 or int(n_beams) < 1 or int(beam_first) < 0:
        raise ValueError(f"pool >= 1, n_beams >= 1, beam_first >= 0: got {pool}, {n_beams}, {beam_first}")
    if not (np.isfinite(max_range) and max_range > 0):
        raise ValueError(f"max_range must be finite and > 0, got {max_range}")
    n_in = int(n_beams) + (NET_STATE_INPUTS if use_state else 0) + n_frame + n_rival
    if n_in > NET_MAX_INPUTS:
        raise ValueError(f"n_beams + 5 use_state + {n_frame} frame entries + {n_rival} rival entries = {n_in} inputs, at most {NET_MAX_INPUTS}")
    for name, act in (("hidden_act", hidden_act), ("out_act", out_act)):
        if act not in ACT_BY_NAME:
            raise ValueError(f"{name}: one of {sorted(ACT_BY_NAME)}, got {act!r}")
    scale, offset = np.asarray(out_scale, dtype=np.float32), np.asarray(out_offset, dtype=np.float32)
    if scale.shape != (2,) or offset.shape != (2,) or not (np.isfinite(scale).all() and np.isfinite(offset).all()):
        raise ValueError("out_scale and out_offset: two finite numbers each")
    d = FtgpNetDesc(pool=int(pool), max_range=float(max_range), beam_first=int(beam_first), n_beams=int(n_beams),
                    use_state=1 if use_state else 0, n_layers=len(layers), hidden_act=ACT_BY_NAME[hidden_act], out_act=ACT_BY_NAME[out_act])
    flat, width = [], n_in
    for l, (W, b) in enumerate(layers):
        last = l == len(layers) - 1
        if W.ndim != 2 or W.shape[1] != width or b.shape != (W.shape[0],):
            raise ValueError(f"layer {l}: W [n_out, {width}] and b [n_out] (torch's nn.Linear layout), got {W.shape} and {b.shape}")
        if last and W.shape[0] != 2:
            raise ValueError(f"the last layer has exactly 2 outputs (speed, steering_angle), got {W.shape[0]}")
        if not last and not 1 <= W.shape[0] <= NET_MAX_HIDDEN:
            raise ValueError(f"layer {l}: a hidden width is 1 .. {NET_MAX_HIDDEN}, got {W.shape[0]}")
        d.width[l] = width = W.shape[0]
        flat += [W.ravel(), b.ravel()]
    for k in range(2):
        d.out_scale[k], d.out_offset[k] = float(scale[k]), float(offset[k])
    return d, np.ascontiguousarray(np.concatenate(flat), dtype=np.float32)


def check_net_window(n_rays: int, pool: int, beam_first: int, n_beams: int):
    """The window rule of ftgp_set_net (ValueError): the device drivers see rays [eighth, n_rays - eighth) only."""
    eighth = int(n_rays / 8.0)
    if n_rays % pool:
        raise ValueError(f"pool {pool} does not divide n_rays {n_rays}")
    if beam_first * pool < eighth or (beam_first + n_beams) * pool > n_rays - eighth:
        raise ValueError(f"beams {beam_first} .. {beam_first + n_beams - 1} of pool {pool} leave the drivers' scan window, "
                         f"rays [{eighth}, {n_rays - eighth}) of {n_rays}: the rear quarter of the scan is not an input")


def net_param_count(d: FtgpNetDesc, frame=None, rivals=None) -> int:
    n, n_in = 0, d.n_beams + (NET_STATE_INPUTS if d.use_state else 0) + net_frame_inputs(frame) + net_rival_inputs(rivals)
    for l in range(d.n_layers):
        n, n_in = n + d.width[l] * n_in + d.width[l], d.width[l]
    return n


def net_layers(d: FtgpNetDesc, flat: np.ndarray, frame=None, rivals=None) -> list:
    """The (W, b) pairs of a flat parameter buffer in ftgp_set_net's layout (``frame``, ``rivals``: the slot's FtgpNetFrame and
    FtgpNetRivals, if it has them)."""
    out, o, n_in = [], 0, d.n_beams + (NET_STATE_INPUTS if d.use_state else 0) + net_frame_inputs(frame) + net_rival_inputs(rivals)
    for l in range(d.n_layers):
        n_out = d.width[l]
        W = flat[o:o + n_out * n_in].reshape(n_out, n_in); o += n_out * n_in
        out.append((W.copy(), flat[o:o + n_out].copy())); o += n_out
        n_in = n_out
    return out


def net_population_args(params, env_member, n_envs: int, count=None):
    """(params float32 [n_members, count], env_member int32 [n_envs] or None) of ftgp_set_net_population with every check that needs no
    handle (ValueError): a two-dimensional float32 array of 1 .. n_envs rows -- ``count`` columns where the caller knows the slot's
    count --, and a map of n_envs integers in [0, n_members).  ``params=None`` is the population's removal: (None, None)."""
    if params is None:
        if env_member is not None:
            raise ValueError("env_member without params: a population is removed with params=None alone")
        return None, None
    p = np.asarray(params)
    if p.dtype != np.float32:
        raise ValueError(f"params: float32 [n_members, count], got dtype {p.dtype}")
    if p.ndim != 2 or p.shape[1] < 1:
        raise ValueError(f"params: float32 [n_members, count], got shape {p.shape}")
    if not 1 <= p.shape[0] <= int(n_envs):
        raise ValueError(f"params: 1 .. n_envs = {int(n_envs)} members, got {p.shape[0]}")
    if count is not None and p.shape[1] != int(count):
        raise ValueError(f"params: the slot's networks have {int(count)} parameters, got rows of {p.shape[1]}")
    if env_member is None:
        return np.ascontiguousarray(p), None
    m = np.asarray(env_member)
    if m.dtype == np.bool_ or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"env_member: integers [n_envs], got dtype {m.dtype}")
    if m.shape != (int(n_envs),):
        raise ValueError(f"env_member: one member per env, shape ({int(n_envs)},), got {m.shape}")
    if m.size and (m.min() < 0 or m.max() >= p.shape[0]):
        raise ValueError(f"env_member: entries in [0, n_members = {p.shape[0]}), got {int(m.min())} .. {int(m.max())}")
    return np.ascontiguousarray(p), np.ascontiguousarray(m, dtype=np.int32)


class FtgpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ftgp error {code}: {msg}")
        self.code = code


def product_library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libftgp.so")


class CLib:
    """One loaded shared library exposing the ftgp C-ABI under ``prefix``."""

    def __init__(self, path: str, prefix: str = "ftgp_"):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(the HIP library is required; there is no CPU fallback)")
        self.path, self.prefix = path, prefix
        self.dll = C.CDLL(path)
        self._sig()

    def fn(self, name: str):
        return getattr(self.dll, self.prefix + name)

    def has(self, name: str) -> bool:
        return hasattr(self.dll, self.prefix + name)

    def _sig(self):
        vp, i32, dp = C.c_void_p, C.c_int, C.c_void_p
        sigs = {
            "default_vehicle": (None, [C.POINTER(FtgpVehicle)]),
            "tricycle_vehicle": (None, [C.POINTER(FtgpVehicle)]),
            "last_error": (C.c_char_p, []),
            "create": (i32, [C.POINTER(FtgpConfig), C.POINTER(vp)]),
            "destroy": (i32, [vp]),
            "reset": (i32, [vp, dp]),
            "set_ctrl": (i32, [vp, dp, dp]),
            "step": (i32, [vp, i32]),
            "rollout": (i32, [vp, i32, i32]),
            "set_car_policies": (i32, [vp, dp]),
            "get_lidar": (i32, [vp, dp]),
            "get_snapshot": (i32, [vp, dp]),
            "get_pose": (i32, [vp, dp]),
            "get_progress": (i32, [vp, dp]),
            "get_winners": (i32, [vp, dp]),
            "get_lap_times": (i32, [vp, dp, dp]),
            "get_ctrl": (i32, [vp, dp]),
            "get_race_steps": (i32, [vp, dp]),
            "get_steps": (i32, [vp, dp]),
            "set_pose": (i32, [vp, dp]),
            "policy_eval": (i32, [vp, i32, dp, dp]),
            "eval_progress": (i32, [vp]),
            "metrics_local": (i32, [vp, dp]),
            "device_count": (i32, []),
            "comm_unique_id": (i32, [dp]),
            "comm_init": (i32, [vp, dp, i32, i32]),
            "metrics_allgather": (i32, [vp, dp]),
            "metrics_allgather_begin": (i32, [vp]),
            "metrics_allgather_end": (i32, [vp, dp]),
            "get_distance_field": (i32, [vp, dp]),
            "fakelidar": (i32, [i32, dp, i32, i32, i32, dp, i32, dp, dp, C.c_double, dp, dp]),
            "last_kernel_ms": (i32, [vp, C.POINTER(C.c_float)]),
            "kernel_name": (C.c_char_p, [vp]),
            "selftest": (i32, [i32, C.POINTER(C.c_int64)]),
            "build_info": (C.c_char_p, []),
            "device_io_config": (i32, [vp, C.POINTER(FtgpDeviceIoConfig)]),
            "step_device": (i32, [vp, C.POINTER(FtgpDeviceStep)]),
            "device_io_signals": (i32, [vp, C.POINTER(FtgpDeviceSignals)]),
            "step_device_ex": (i32, [vp, C.POINTER(FtgpDeviceStep), C.POINTER(FtgpDeviceStepExtra)]),
            "state_device": (i32, [vp, vp, vp]),
            "get_centre_dist2": (i32, [vp, dp]),
            "device_io_contacts": (i32, [vp, C.POINTER(FtgpDeviceContacts)]),
            "step_device_contacts": (i32, [vp, C.POINTER(FtgpDeviceStep), C.POINTER(FtgpDeviceStepExtra), C.POINTER(FtgpDeviceStepContacts)]),
            "contacts_device": (i32, [vp, vp, vp]),
            "get_contacts": (i32, [vp, dp]),
            "device_io_frame": (i32, [vp, C.POINTER(FtgpDeviceFrame)]),
            "step_device_frame": (i32, [vp, C.POINTER(FtgpDeviceStep), C.POINTER(FtgpDeviceStepExtra), C.POINTER(FtgpDeviceStepContacts),
                                        C.POINTER(FtgpDeviceStepFrame)]),
            "frame_device": (i32, [vp, vp, vp]),
            "get_frames": (i32, [vp, i32, i32, dp]),
            "device_io_rivals": (i32, [vp, C.POINTER(FtgpDeviceRivals)]),
            "step_device_rivals": (i32, [vp, C.POINTER(FtgpDeviceStep), C.POINTER(FtgpDeviceStepExtra), C.POINTER(FtgpDeviceStepContacts),
                                         C.POINTER(FtgpDeviceStepFrame), C.POINTER(FtgpDeviceStepRivals)]),
            "rivals_device": (i32, [vp, vp, vp]),
            "get_rivals": (i32, [vp, i32, dp]),
            "set_spawn_rule": (i32, [vp, C.POINTER(FtgpSpawnRule)]),
            "get_episodes": (i32, [vp, dp]),
            "get_start_table": (i32, [vp, i32, dp]),
            "set_dynamics": (i32, [vp, dp, dp]),
            "set_dynamics_device": (i32, [vp, vp, vp, vp]),
            "get_dynamics": (i32, [vp, dp, C.POINTER(C.c_int64)]),
            "env_state_bytes": (i32, [vp, C.POINTER(C.c_size_t)]),
            "save_envs_device": (i32, [vp, vp, vp, C.c_int64, vp]),
            "load_envs_device": (i32, [vp, vp, vp, C.c_int64, vp]),
            "get_env_state_rejected": (i32, [vp, C.POINTER(C.c_int64)]),
            "obs_device": (i32, [vp, vp, vp]),
            "set_net": (i32, [vp, i32, C.POINTER(FtgpNetDesc), dp]),
            "set_net_device": (i32, [vp, vp, i32, vp]),
            "get_net": (i32, [vp, i32, C.POINTER(FtgpNetDesc), dp]),
            "set_net_frame": (i32, [vp, i32, C.POINTER(FtgpNetDesc), C.POINTER(FtgpNetFrame), dp]),
            "get_net_frame": (i32, [vp, i32, C.POINTER(FtgpNetFrame)]),
            "set_net_rivals": (i32, [vp, i32, C.POINTER(FtgpNetDesc), C.POINTER(FtgpNetFrame), C.POINTER(FtgpNetRivals), dp]),
            "get_net_rivals": (i32, [vp, i32, C.POINTER(FtgpNetRivals)]),
            "collect_device": (i32, [vp, C.POINTER(FtgpCollect)]),
            "set_net_population": (i32, [vp, i32, i32, dp, dp]),
            "set_net_population_device": (i32, [vp, vp, i32, vp, vp]),
            "get_net_population": (i32, [vp, i32, C.POINTER(C.c_int32), dp, i32, dp]),
            "set_value_net": (i32, [vp, i32, C.POINTER(FtgpValueDesc), dp]),
            "set_value_net_device": (i32, [vp, vp, i32, vp]),
            "get_value_net": (i32, [vp, i32, C.POINTER(FtgpValueDesc), dp]),
            "collect_values_device": (i32, [vp, C.POINTER(FtgpCollect), C.POINTER(FtgpCollectValues)]),
            "gae_device": (i32, [vp, vp, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp]),
            "train_begin": (i32, [vp, i32, C.POINTER(FtgpTrainDesc)]),
            "train_end": (i32, [vp, i32]),
            "train_grad_device": (i32, [vp, C.POINTER(FtgpTrainBatch)]),
            "train_adam_device": (i32, [vp, vp, i32, C.c_float]),
            "train_get": (i32, [vp, i32, i32, dp, dp, C.POINTER(C.c_int64)]),
            "create_tracks": (i32, [C.POINTER(FtgpConfig), C.POINTER(FtgpTrack), dp, i32, C.POINTER(vp)]),
            "get_track_distance_field": (i32, [vp, i32, dp]),
        }
        for name, (res, args) in sigs.items():
            if name == "fakelidar" and self.prefix != "ftgp_":
                continue        # the oracle's single-origin form is typed by tests/helpers.py
            if self.has(name):
                f = self.fn(name)
                f.restype, f.argtypes = res, args

    def build_info(self) -> dict:
        """What the library says it was built from and with (ftgp_build_info): {"abi", "sources", "diag", ...}."""
        text = self.fn("build_info")().decode()
        return dict(kv.split("=", 1) for kv in text.split() if "=" in kv) | {"diag": text.split("diag=", 1)[1].split(" fair_shift=")[0]}

    def last_error(self) -> str:
        s = self.fn("last_error")()
        return s.decode() if s else ""

    def check(self, code: int):
        if code != 0:
            raise FtgpError(code, self.last_error())

    def default_vehicle(self) -> FtgpVehicle:
        v = FtgpVehicle()
        self.fn("default_vehicle")(C.byref(v))
        return v

    def tricycle_vehicle(self) -> FtgpVehicle:
        """The legacy differential-drive car of template/car.em.xml (pair it with dt = 0.0075)."""
        v = FtgpVehicle()
        self.fn("tricycle_vehicle")(C.byref(v))
        return v


_product: Optional[CLib] = None


def load() -> CLib:
    """The product library (HIP).  Raises if it has not been built."""
    global _product
    if _product is None:
        _product = CLib(product_library_path(), "ftgp_")
    return _product


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def split_envs(n_envs: int, n_tracks: int) -> tuple:
    """The default envs_per_track of a multi-track handle: as even as possible, the remainder to the first blocks."""
    n_envs, n_tracks = int(n_envs), int(n_tracks)
    return tuple(n_envs // n_tracks + (1 if t < n_envs % n_tracks else 0) for t in range(n_tracks))


def track_blocks(n_envs: int, n_tracks: int, envs_per_track=None) -> tuple:
    """envs_per_track of a multi-track handle, checked (ValueError): 1 <= n_tracks <= MAX_TRACKS, one count >= 1 per track, summing to
    n_envs; None = ``split_envs``."""
    n_envs, n_tracks = int(n_envs), int(n_tracks)
    if not 1 <= n_tracks <= MAX_TRACKS:
        raise ValueError(f"a handle holds 1 .. {MAX_TRACKS} tracks, got {n_tracks}")
    if envs_per_track is None:
        if n_envs < n_tracks:
            raise ValueError(f"{n_envs} envs cannot give each of {n_tracks} tracks an env")
        return split_envs(n_envs, n_tracks)
    counts = tuple(int(c) for c in envs_per_track)
    if len(counts) != n_tracks:
        raise ValueError(f"envs_per_track: one count per track, expected {n_tracks}, got {len(counts)}")
    if min(counts) < 1:
        raise ValueError(f"envs_per_track: every track needs at least one env, got {counts}")
    if sum(counts) != n_envs:
        raise ValueError(f"envs_per_track sums to {sum(counts)}, n_envs is {n_envs}")
    return counts


def _fill_track(t: FtgpTrack, track) -> tuple:
    """Fill the C struct from a Track; returns the arrays it points into (keep them alive)."""
    bits = np.ascontiguousarray(track.bits, dtype=np.uint32)
    path = np.ascontiguousarray(track.path, dtype=np.float64)
    assert path.shape == (PATH_POINTS, 2)
    t.width, t.height, t.words_per_row = track.width, track.height, bits.shape[1]
    t.bits, t.path = bits.ctypes.data, path.ctypes.data
    t.px_size_x, t.px_size_y, t.origin_x, t.origin_y = track.px_size_x, track.px_size_y, track.origin_x, track.origin_y
    return bits, path


class Env:
    """A batch of worlds behind one opaque C handle (see include/ftgp.h for the contract of each call).

    track: one Track (ftgp_create), or a list / tuple of Tracks (ftgp_create_tracks): env block t = envs_per_track[t] consecutive envs
    on track t, as even a split as possible by default (``split_envs``).  ``tracks`` lists the tracks, ``track_of_env`` (int32 [n_envs])
    says which track each env races; ``track`` is the first."""

    def __init__(self, lib: CLib, track: Track, n_envs: int = 1, cars_per_env: int = 1, n_rays: int = 90,
                 lap_target: int = 10, dt: float = 0.004, spawn_mode: int = 0, seed: int = 1234,
                 device_id: int = 0, vehicle: Optional[FtgpVehicle] = None, env_base: int = 0,
                 bubble_wrap: bool = False, naive_flatten: bool = False, lidar_mode="rangefinder", map_size: float = 0.0,
                 fan_dirs: Optional[np.ndarray] = None, envs_per_track=None):
        multi = isinstance(track, (list, tuple))
        tracks = list(track) if multi else [track]
        if multi:
            counts = track_blocks(n_envs, len(tracks), envs_per_track)
        elif envs_per_track is not None:
            raise ValueError("envs_per_track needs a list of tracks")
        else:
            counts = (int(n_envs),)
        self.lib, self.track, self.tracks, self.envs_per_track = lib, tracks[0], tracks, counts
        self.track_of_env = np.repeat(np.arange(len(tracks), dtype=np.int32), counts)
        self.n_envs, self.cars_per_env, self.n_rays = int(n_envs), int(cars_per_env), int(n_rays)
        self.n_cars = self.n_envs * self.cars_per_env
        self.dt, self.lap_target = float(dt), int(lap_target)
        cfg = FtgpConfig()
        cfg.abi_version = ABI_VERSION
        cfg.n_envs, cfg.cars_per_env, cfg.n_rays = self.n_envs, self.cars_per_env, self.n_rays
        cfg.lap_target, cfg.device_id, cfg.spawn_mode, cfg.seed, cfg.dt = lap_target, device_id, spawn_mode, seed, dt
        cfg.env_base = env_base
        cfg.bubble_wrap, cfg.naive_flatten = int(bool(bubble_wrap)), int(bool(naive_flatten))
        cfg.lidar_mode = LIDAR_BY_NAME[lidar_mode] if isinstance(lidar_mode, str) else int(lidar_mode)
        cfg.map_size = float(map_size)
        self._fan = None if fan_dirs is None else np.ascontiguousarray(fan_dirs, dtype=np.float64).reshape(self.n_rays, 2)
        cfg.fan_dirs = None if self._fan is None else self._fan.ctypes.data
        self.env_base = int(env_base)
        cfg.vehicle = vehicle if vehicle is not None else lib.default_vehicle()
        self.cfg = cfg
        self.h = C.c_void_p()
        if not multi:
            self._bits, self._path = _fill_track(cfg.track, track)
            lib.check(lib.fn("create")(C.byref(cfg), C.byref(self.h)))
        else:
            self._tracks = (FtgpTrack * len(tracks))()
            self._keep = [_fill_track(self._tracks[k], t) for k, t in enumerate(tracks)]
            self._counts = np.array(counts, dtype=np.int32)
            lib.check(lib.fn("create_tracks")(C.byref(cfg), self._tracks, _ptr(self._counts), len(tracks), C.byref(self.h)))

    # -- lifecycle
    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _call(self, name, *args):
        self.lib.check(self.lib.fn(name)(self.h, *args))

    # -- control
    def reset(self, mask: Optional[np.ndarray] = None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None:
            assert m.shape == (self.n_envs,)
        self._call("reset", _ptr(m))

    def set_ctrl(self, ctrl: np.ndarray, car_mask: Optional[np.ndarray] = None):
        c = np.ascontiguousarray(ctrl, dtype=np.float64).reshape(self.n_cars, 2)
        m = None if car_mask is None else np.ascontiguousarray(car_mask, dtype=np.uint8).reshape(self.n_cars)
        self._call("set_ctrl", _ptr(c), _ptr(m))

    def step(self, n_steps: int = 1):
        self._call("step", int(n_steps))

    def rollout(self, policy, n_steps: int):
        p = POLICY_BY_NAME[policy] if isinstance(policy, str) else int(policy)
        self._call("rollout", p, int(n_steps))

    def set_car_policies(self, policies):
        """The bundled driver of every car slot of an env (names or numbers, one per car of the roster): what
        ``rollout("per_car", n)`` evaluates.  Replaces the per-vehicle Driver() instances of custom.py:1097-1104."""
        p = np.array([POLICY_BY_NAME[x] if isinstance(x, str) else int(x) for x in policies], dtype=np.int32)
        if p.shape != (self.cars_per_env,):
            raise ValueError(f"one policy per car of an env: expected {self.cars_per_env}, got {p.shape}")
        self._call("set_car_policies", _ptr(p))

    # -- device I/O (include/ftgp.h: ftgp_device_io_config / ftgp_step_device); ft_grandprix_amd.vec wraps it on torch tensors
    def device_io_config(self, roster=None, max_episode_steps: int = 0, action_repeat: int = 1, auto_reset: bool = True):
        """roster: one entry per car slot ("host"/"agent" = external, or a bundled driver), None = every slot external."""
        cfg = FtgpDeviceIoConfig()
        r = None
        if roster is not None:
            r = np.array([POLICY_HOST if x == "agent" else POLICY_BY_NAME[x] if isinstance(x, str) else int(x) for x in roster],
                         dtype=np.int32)
            if r.shape != (self.cars_per_env,):
                raise ValueError(f"one roster entry per car of an env: expected {self.cars_per_env}, got {r.shape}")
            cfg.roster = r.ctypes.data
        cfg.max_episode_steps, cfg.action_repeat, cfg.auto_reset = int(max_episode_steps), int(action_repeat), int(bool(auto_reset))
        self._call("device_io_config", C.byref(cfg))

    def device_io_signals(self, scan_pool: int = 1, scan_max_range: float = 0.0, terminate_off_track: bool = False,
                          off_track_penalty: float = 0.0):
        """ftgp_device_io_signals (after ``device_io_config``, which puts the defaults back): pooled / scaled scans, off-track ends."""
        s = FtgpDeviceSignals(int(scan_pool), float(scan_max_range), int(bool(terminate_off_track)), float(off_track_penalty))
        self._call("device_io_signals", C.byref(s))

    def device_io_contacts(self, on: bool = True, terminate_on_wall: bool = False, terminate_on_car: bool = False,
                           wall_penalty: float = 0.0, car_penalty: float = 0.0):
        """ftgp_device_io_contacts (after ``device_io_config``, which turns contacts off): contact rows, contact episode ends and
        penalties in every device step; ``on=False`` turns them off again."""
        if not on:
            self._call("device_io_contacts", None)
            return
        c = FtgpDeviceContacts(int(bool(terminate_on_wall)), int(bool(terminate_on_car)), float(wall_penalty), float(car_penalty))
        self._call("device_io_contacts", C.byref(c))

    def device_io_frame(self, on: bool = True, n_ahead: int = 0, stride: int = 1, dense_progress: bool = False):
        """ftgp_device_io_frame (after ``device_io_config``, which turns the frame off): a track-frame row per car in every device step
        (FRAME_FIELDS, then ``n_ahead`` look-ahead points ``stride`` path points apart, body frame), and with ``dense_progress`` the
        change of the continuous lap position as the reward; ``on=False`` turns it off again."""
        if not on:
            self._call("device_io_frame", None)
            return
        f = FtgpDeviceFrame(int(n_ahead), int(stride), int(bool(dense_progress)), 0)
        self._call("device_io_frame", C.byref(f))

    def device_io_rivals(self, on: bool = True, n_rivals: int = 0, place_weight: float = 0.0):
        """ftgp_device_io_rivals (after ``device_io_config``, which turns rivals off): a rival row per car in every device step
        (RIVAL_FIELDS, then ``n_rivals`` mate slots of RIVAL_MATE_FIELDS, nearest mate first), and with ``place_weight`` w > 0 the
        places gained over the call, times w, on top of the reward; ``on=False`` turns them off again."""
        if not on:
            self._call("device_io_rivals", None)
            return
        r = FtgpDeviceRivals(int(n_rivals), 0, float(place_weight), 0.0)
        self._call("device_io_rivals", C.byref(r))

    # -- spawn rule (include/ftgp.h: ftgp_set_spawn_rule)
    def set_spawn_rule(self, on: bool = True, first_point: int = 0, n_points: int = PATH_POINTS, margin: float = 0.0,
                       lateral_frac: float = 0.0, yaw_tan: float = 0.0, shuffle_grid: bool = False):
        """ftgp_set_spawn_rule: from now on every reset -- ``reset`` with or without a mask, the auto-reset of a device step -- draws
        start point, lateral offset, yaw (``yaw_tan`` = tan of half the largest offset) and grid order per (seed, env, episode);
        ``on=False`` puts the fixed starts of ``spawn_mode`` back.  Every call zeroes ``episodes()``."""
        if not on:
            self._call("set_spawn_rule", None)
            return
        r = FtgpSpawnRule(int(first_point), int(n_points), int(bool(shuffle_grid)), 0, float(margin), float(lateral_frac), float(yaw_tan))
        self._call("set_spawn_rule", C.byref(r))

    def episodes(self) -> np.ndarray:
        """int64 [n_envs]: resets of every env since the spawn rule was set (zeros without a rule)."""
        out = np.empty(self.n_envs, dtype=np.int64)
        self._call("get_episodes", _ptr(out))
        return out

    def start_table(self, track: int = 0) -> np.ndarray:
        """float64 [100, 6] of track ``track``: x, y, qw, qz of the spawn table, wall clearance to the left and to the right."""
        track = int(track)
        if not 0 <= track < len(self.tracks):
            raise ValueError(f"track {track} of a handle with {len(self.tracks)}")
        out = np.empty((PATH_POINTS, 6), dtype=np.float64)
        self._call("get_start_table", track, _ptr(out))
        return out

    # -- per-car dynamics (include/ftgp.h: ftgp_set_dynamics)
    def base_dynamics(self) -> np.ndarray:
        """float64 [DYN_DOUBLES]: the handle's own dynamics row, i.e. the DYN_FIELDS of its vehicle."""
        return np.array([getattr(self.cfg.vehicle, f) for f in DYN_FIELDS], dtype=np.float64)

    def set_dynamics(self, rows, env_mask: Optional[np.ndarray] = None):
        """ftgp_set_dynamics: ``rows`` float64 [n_envs, cars_per_env, DYN_DOUBLES] (DYN_FIELDS) become the dynamics of the cars of the
        envs ``env_mask`` (uint8 [n_envs], None = all) names; the first call turns the table on, every other car starting from the
        handle's own values.  ``rows=None`` turns the table off."""
        if rows is None:
            if env_mask is not None:
                raise ValueError("set_dynamics(None) takes no mask")
            self._call("set_dynamics", None, None)
            return
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.size != self.n_cars * DYN_DOUBLES:
            raise ValueError(f"rows: {self.n_cars} x {DYN_DOUBLES} values, got shape {r.shape}")
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        if m is not None and m.shape != (self.n_envs,):
            raise ValueError(f"env_mask: one byte per env, expected ({self.n_envs},), got {m.shape}")
        self._call("set_dynamics", _ptr(r), _ptr(m))

    def set_dynamics_device(self, rows_ptr: int, env_mask_ptr: int = 0, stream: int = 0):
        """ftgp_set_dynamics_device on integer device addresses (float64 [n_envs, cars_per_env, DYN_DOUBLES], uint8 [n_envs] or 0 = all
        envs), ordered on ``stream``; only enqueues.  A car whose row is invalid keeps its old one (``dynamics()[1]`` counts them)."""
        self._call("set_dynamics_device", stream or None, rows_ptr or None, env_mask_ptr or None)

    def dynamics(self):
        """(rows, rejected): float64 [n_cars, DYN_DOUBLES], the dynamics row in force for every car (the handle's own values while the
        table is off), and the number of rows the device setter has rejected since the table was turned on."""
        out = np.empty((self.n_cars, DYN_DOUBLES), dtype=np.float64)
        rejected = C.c_int64(0)
        self._call("get_dynamics", _ptr(out), C.byref(rejected))
        return out, int(rejected.value)

    # -- network drivers (include/ftgp.h: ftgp_set_net)
    def set_net(self, slot: int, layers, *, pool=None, max_range=None, beam_first=None, n_beams=None, use_state=False,
                hidden_act="tanh", out_act="tanh", out_scale=(1, 1), out_offset=(0, 0), frame=False, lookahead=0, lookahead_stride=1,
                rivals=False, n_rivals=0):
        """ftgp_set_net / ftgp_set_net_frame / ftgp_set_net_rivals: ``layers`` = [(W [n_out, n_in], b [n_out]), ...] (torch's nn.Linear layout) becomes the
        network driver ``"net<slot>"``; ``layers=None`` clears the slot.  ``frame`` (or ``lookahead > 0``): the track-frame row with
        ``lookahead`` points every ``lookahead_stride`` path points follows the beams and the state inputs.  ``rivals`` (or
        ``n_rivals > 0``): the rival row of the car's env with ``n_rivals`` mate slots follows those."""
        if layers is None:
            self._call("set_net", int(slot), None, None)
            return
        d, flat = net_desc(layers, pool=pool, max_range=max_range, beam_first=beam_first, n_beams=n_beams, use_state=use_state,
                           hidden_act=hidden_act, out_act=out_act, out_scale=out_scale, out_offset=out_offset,
                           frame=frame, lookahead=lookahead, lookahead_stride=lookahead_stride, rivals=rivals, n_rivals=n_rivals)
        f = net_frame(frame, lookahead, lookahead_stride)
        r = net_rivals(rivals, n_rivals)
        if r.enabled:
            self._call("set_net_rivals", int(slot), C.byref(d), C.byref(f), C.byref(r), _ptr(flat))
        elif f.enabled:
            self._call("set_net_frame", int(slot), C.byref(d), C.byref(f), _ptr(flat))
        else:
            self._call("set_net", int(slot), C.byref(d), _ptr(flat))

    def set_net_device(self, slot: int, address: int, stream: int = 0):
        """ftgp_set_net_device: new parameters for a defined slot from the integer device address of a float32 buffer in
        ftgp_set_net's flat layout, ordered on ``stream``; only enqueues."""
        self._call("set_net_device", stream or None, int(slot), address or None)

    def net(self, slot: int):
        """(FtgpNetDesc, [(W, b), ...]): the description and the parameters in force of a defined slot (ftgp_get_net)."""
        d, f, r = FtgpNetDesc(), FtgpNetFrame(), FtgpNetRivals()
        self._call("get_net", int(slot), C.byref(d), None)
        self._call("get_net_frame", int(slot), C.byref(f))
        self._call("get_net_rivals", int(slot), C.byref(r))
        flat = np.empty(net_param_count(d, f, r), dtype=np.float32)
        self._call("get_net", int(slot), C.byref(d), _ptr(flat))
        return d, net_layers(d, flat, f, r)

    def net_frame(self, slot: int) -> dict:
        """The frame inputs of a defined slot (ftgp_get_net_frame): ``dict(frame, lookahead, lookahead_stride)``, set_net's keywords."""
        f = FtgpNetFrame()
        self._call("get_net_frame", int(slot), C.byref(f))
        return dict(frame=bool(f.enabled), lookahead=int(f.n_ahead), lookahead_stride=int(f.stride) if f.enabled else 1)

    def net_rivals(self, slot: int) -> dict:
        """The rival inputs of a defined slot (ftgp_get_net_rivals): ``dict(rivals, n_rivals)``, set_net's keywords."""
        r = FtgpNetRivals()
        self._call("get_net_rivals", int(slot), C.byref(r))
        return dict(rivals=bool(r.enabled), n_rivals=int(r.n_rivals))

    def get_net(self, slot: int):
        """(FtgpNetDesc, [(W, b), ...], dict(frame, lookahead, lookahead_stride)): ``net`` and ``net_frame`` of a defined slot; for a slot
        with rival inputs the dict has ``net_rivals``' two fields (rivals, n_rivals) as well -- set_net's keywords, so
        ``set_net(slot, layers, **fields_of_the_description, **that_dict)`` defines the same slot again."""
        r = self.net_rivals(slot)
        return self.net(slot) + ({**self.net_frame(slot), **(r if r["rivals"] else {})},)

    # -- network populations (include/ftgp.h: ftgp_set_net_population)
    def _net_count(self, slot: int) -> int:
        """Floats of a defined slot's parameters in the caller's layout, from its description alone (nothing is read back)."""
        d, f, r = FtgpNetDesc(), FtgpNetFrame(), FtgpNetRivals()
        self._call("get_net", int(slot), C.byref(d), None)
        self._call("get_net_frame", int(slot), C.byref(f))
        self._call("get_net_rivals", int(slot), C.byref(r))
        return net_param_count(d, f, r)

    def set_net_population(self, slot: int, params, env_member=None):
        """ftgp_set_net_population: ``params`` float32 [n_members, count] -- one row per member in ftgp_set_net's flat layout
        (``NetSpec.flat_params``, ``net.stack_params``) -- and ``env_member`` int32 [n_envs] (None: env e gets member e % n_members) make
        defined slot ``slot`` a population: env e's cars driven by ``"net<slot>"`` run member env_member[e].  ``params=None`` removes it."""
        p, m = net_population_args(params, env_member, self.n_envs)
        if p is None:
            self._call("set_net_population", int(slot), 0, None, None)
            return
        net_population_args(p, None, self.n_envs, self._net_count(slot))      # (a slot that is not defined: the library's message)
        self._call("set_net_population", int(slot), int(p.shape[0]), _ptr(p), _ptr(m) if m is not None else None)

    def set_net_population_device(self, slot: int, params_address: int, env_member_address: int = 0, stream: int = 0):
        """ftgp_set_net_population_device: new parameters (float32 [n_members, count]) and / or a new map (int32 [n_envs]) for a slot
        that carries a population, from integer device addresses (0 = keep), ordered on ``stream``; only enqueues.  A map entry
        outside [0, n_members) is taken as member 0."""
        self._call("set_net_population_device", stream or None, int(slot), params_address or None, env_member_address or None)

    def get_net_population(self, slot: int, member=None):
        """ftgp_get_net_population: (n_members, env_member int32 [n_envs]) of a defined slot -- (0, None) without a population --, or,
        with ``member``, that member's flat float32 parameters."""
        n = C.c_int32(0)
        self._call("get_net_population", int(slot), C.byref(n), None, 0, None)
        if member is None:
            if n.value == 0:
                return 0, None
            m = np.empty(self.n_envs, dtype=np.int32)
            self._call("get_net_population", int(slot), None, _ptr(m), 0, None)
            return int(n.value), m
        flat = np.empty(self._net_count(slot), dtype=np.float32)
        self._call("get_net_population", int(slot), None, None, int(member), _ptr(flat))
        return flat

    # -- collected rollouts (include/ftgp.h: ftgp_collect_device)
    def collect_device(self, n_decisions: int, inputs: int, mean: int, action: int, reward: int, terminated: int, truncated: int, *,
                       slot: int = 0, std=(0.0, 0.0), clip=((-1e30, 1e30), (-1e30, 1e30)), noise: int = 0, next_inputs: int = 0,
                       reset_dynamics: int = 0, stream: int = 0):
        """One ftgp_collect_device call on integer device addresses (0 = NULL for the optional ``noise``, ``next_inputs`` and
        ``reset_dynamics``), ordered on ``stream``; only enqueues.  ``n_decisions`` decisions of network slot ``slot`` for every
        external car; the buffers hold ``n_decisions`` times the rows of one decision."""
        c = collect_args(n_decisions, slot, std, clip)
        c.stream = stream or None
        for name, v in (("noise", noise), ("inputs", inputs), ("mean", mean), ("action", action), ("reward", reward),
                        ("terminated", terminated), ("truncated", truncated), ("next_inputs", next_inputs),
                        ("reset_dynamics", reset_dynamics)):
            setattr(c, name, v or None)
        self._call("collect_device", C.byref(c))

    # -- collected rollouts with values (include/ftgp.h: ftgp_set_value_net, ftgp_collect_values_device, ftgp_gae_device)
    def set_value_net(self, slot: int, layers, *, hidden_act="tanh", out_act="identity", out_scale=1.0, out_offset=0.0):
        """ftgp_set_value_net: ``layers`` = [(W [n_out, n_in], b [n_out]), ...] with one output becomes the value net of defined slot
        ``slot`` -- it reads the slot's own input vector; ``layers=None`` clears it."""
        if layers is None:
            self._call("set_value_net", int(slot), None, None)
            return
        d, flat = value_desc(layers, hidden_act=hidden_act, out_act=out_act, out_scale=out_scale, out_offset=out_offset)
        n_in = self._net_n_in(slot)            # (a slot that is not defined: the library's message)
        if np.asarray(layers[0][0]).shape[1] != n_in:
            raise ValueError(f"layer 0: the value net reads slot {int(slot)}'s {n_in} inputs, got W with {np.asarray(layers[0][0]).shape[1]} columns")
        self._call("set_value_net", int(slot), C.byref(d), _ptr(flat))

    def set_value_net_device(self, slot: int, address: int, stream: int = 0):
        """ftgp_set_value_net_device: new parameters for a slot's value net from the integer device address of a float32 buffer in
        the flat layout, ordered on ``stream``; only enqueues, never synchronises."""
        self._call("set_value_net_device", stream or None, int(slot), address or None)

    def _net_n_in(self, slot: int) -> int:
        d, f, r = FtgpNetDesc(), FtgpNetFrame(), FtgpNetRivals()
        self._call("get_net", int(slot), C.byref(d), None)
        self._call("get_net_frame", int(slot), C.byref(f))
        self._call("get_net_rivals", int(slot), C.byref(r))
        return d.n_beams + (NET_STATE_INPUTS if d.use_state else 0) + net_frame_inputs(f) + net_rival_inputs(r)

    def get_value_net(self, slot: int):
        """(FtgpValueDesc, [(W, b), ...]): the description and the parameters in force of a slot's value net (ftgp_get_value_net)."""
        d = FtgpValueDesc()
        self._call("get_value_net", int(slot), C.byref(d), None)
        n_in = self._net_n_in(slot)
        flat = np.empty(value_param_count(d, n_in), dtype=np.float32)
        self._call("get_value_net", int(slot), C.byref(d), _ptr(flat))
        return d, value_layers(d, flat, n_in)

    def collect_values_device(self, n_decisions: int, inputs: int, mean: int, action: int, reward: int, terminated: int, truncated: int,
                              value: int, next_value: int, *, advantage: int = 0, ret: int = 0, gamma=0.99, lam=0.95,
                              slot: int = 0, std=(0.0, 0.0), clip=((-1e30, 1e30), (-1e30, 1e30)), noise: int = 0, next_inputs: int = 0,
                              reset_dynamics: int = 0, stream: int = 0):
        """One ftgp_collect_values_device call on integer device addresses: ``collect_device`` with the slot's value net evaluated
        into ``value`` and ``next_value`` (float32 [T, n_envs, n_ext]) and, with ``advantage`` and ``ret`` (both or neither, 0 = NULL),
        the advantage scan with ``gamma`` and ``lam`` behind the last decision.  Only enqueues."""
        c = collect_args(n_decisions, slot, std, clip)
        v = collect_values_args(gamma, lam, value, next_value, advantage, ret)
        c.stream = stream or None
        for name, a in (("noise", noise), ("inputs", inputs), ("mean", mean), ("action", action), ("reward", reward),
                        ("terminated", terminated), ("truncated", truncated), ("next_inputs", next_inputs),
                        ("reset_dynamics", reset_dynamics)):
            setattr(c, name, a or None)
        self._call("collect_values_device", C.byref(c), C.byref(v))

    def gae_device(self, n_decisions: int, reward: int, value: int, next_value: int, terminated: int, truncated: int,
                   advantage: int, ret: int, *, gamma=0.99, lam=0.95, stream: int = 0):
        """ftgp_gae_device on integer device addresses: the advantage scan over ``n_decisions`` decisions of the handle's external
        rows, ordered on ``stream``; only enqueues."""
        if isinstance(n_decisions, bool) or not isinstance(n_decisions, (int, np.integer)) or not 1 <= int(n_decisions) < 2 ** 31:
            raise ValueError(f"n_decisions: an integer >= 1, got {n_decisions!r}")
        g, l = check_discounts(gamma, lam)
        self._call("gae_device", stream or None, int(n_decisions), g, l, reward or None, value or None, next_value or None,
                   terminated or None, truncated or None, advantage or None, ret or None)

    # -- training on the device (include/ftgp.h: ftgp_train_begin, ftgp_train_grad_device, ftgp_train_adam_device)
    def train_begin(self, slot: int = 0, betas=(0.9, 0.999), eps=1e-8):
        """ftgp_train_begin: a trainer for defined slot ``slot`` (it needs a value net and no population): zeroed gradient and moments, t = 0."""
        d = train_desc(betas, eps)
        self._call("train_begin", _train_slot(slot), C.byref(d))

    def train_end(self, slot: int = 0):
        self._call("train_end", _train_slot(slot))

    def train_grad_device(self, batch: "FtgpTrainBatch"):
        """ftgp_train_grad_device on a ``train_batch``: the PPO gradient of the batch rows into the trainer's gradient; only enqueues."""
        self._call("train_grad_device", C.byref(batch))

    def train_adam_device(self, slot: int = 0, lr=3e-4, stream: int = 0):
        """ftgp_train_adam_device: one Adam step on the slot's policy and value parameters in place; only enqueues."""
        self._call("train_adam_device", stream or None, _train_slot(slot), _f32("lr", lr, "finite and >= 0", lambda f: f >= 0.0))

    def train_get(self, slot: int = 0, what: int = TRAIN_GRAD):
        """(policy float32 [count], value float32 [count], t): the gradient (TRAIN_GRAD) or a moment (TRAIN_M, TRAIN_V) of both nets in
        ftgp_get_net's flat layout, and the Adam steps taken (synchronous)."""
        slot = _train_slot(slot)
        vd = FtgpValueDesc()
        self._call("get_value_net", slot, C.byref(vd), None)
        pol = np.empty(self._net_count(slot), dtype=np.float32)
        val = np.empty(value_param_count(vd, self._net_n_in(slot)), dtype=np.float32)
        t = C.c_int64(0)
        self._call("train_get", slot, int(what), _ptr(pol), _ptr(val), C.byref(t))
        return pol, val, int(t.value)

    def train_get_raw(self, slot: int = 0, what: int = TRAIN_RAW_GRAD):
        """(policy, value): per net a list of (Wt float32 [n_in, ld], b float32 [ld]) per layer -- the gradient (TRAIN_RAW_GRAD) or the
        parameters in force (TRAIN_RAW_PARAMS) as they lie in device memory, ld = n_out rounded up to 64: a debug read for tests, which
        look at the padding (synchronous)."""
        slot = _train_slot(slot)
        d, vd = FtgpNetDesc(), FtgpValueDesc()
        self._call("get_net", slot, C.byref(d), None)
        self._call("get_value_net", slot, C.byref(vd), None)
        n_in = self._net_n_in(slot)
        out = []
        shapes = [[n_in] + list(x.width[:x.n_layers]) for x in (d, vd)]
        bufs = [np.full(sum((i + 1) * ((o + 63) // 64 * 64) for i, o in zip(w[:-1], w[1:])), np.nan, dtype=np.float32) for w in shapes]
        self._call("train_get", slot, int(what), _ptr(bufs[0]), _ptr(bufs[1]), None)
        for w, buf in zip(shapes, bufs):
            layers, at = [], 0
            for i, o in zip(w[:-1], w[1:]):
                ld = (o + 63) // 64 * 64
                layers.append((buf[at:at + i * ld].reshape(i, ld), buf[at + i * ld:at + (i + 1) * ld]))
                at += (i + 1) * ld
            out.append(layers)
        return tuple(out)

    # -- env states on the device (include/ftgp.h: ftgp_save_envs_device)
    def env_state_bytes(self) -> int:
        """Bytes of one env-state record of this handle (= ``env_state_layout(n_rays, cars_per_env)["bytes"]``)."""
        n = C.c_size_t(0)
        self._call("env_state_bytes", C.byref(n))
        return int(n.value)

    def save_envs_device(self, rows_ptr: int, n_rows: int, env_mask_ptr: int = 0, stream: int = 0):
        """ftgp_save_envs_device on integer device addresses: env e of the mask (uint8 [n_envs], 0 = all envs) writes row e of the
        ``n_rows`` >= n_envs records at ``rows_ptr``; ordered on ``stream``, only enqueues."""
        self._call("save_envs_device", stream or None, rows_ptr or None, int(n_rows), env_mask_ptr or None)

    def load_envs_device(self, rows_ptr: int, n_rows: int, src_row_ptr: int = 0, stream: int = 0):
        """ftgp_load_envs_device on integer device addresses: env e takes row src_row[e] (int32 [n_envs], 0 = row e; a negative entry
        keeps the env) of the ``n_rows`` records at ``rows_ptr``; ordered on ``stream``, only enqueues.  A row that does not fit the env
        leaves it untouched (``env_state_rejected()`` counts them)."""
        self._call("load_envs_device", stream or None, rows_ptr or None, int(n_rows), src_row_ptr or None)

    def env_state_rejected(self) -> int:
        """Rows ftgp_load_envs_device has refused over the handle's life (synchronous)."""
        n = C.c_int64(0)
        self._call("get_env_state_rejected", C.byref(n))
        return int(n.value)

    def obs_device(self, obs: int, stream: int = 0):
        """ftgp_obs_device: the agents' observation rows at the state as it stands into device memory at ``obs`` (float32 [n_envs,
        n_ext, n_beams]), ordered on ``stream``; only enqueues."""
        self._call("obs_device", stream or None, obs or None)

    @staticmethod
    def _step_args(stream, action, obs, reward, terminated, truncated, final_obs, *rows):
        """The arguments of a device step by reference: the FtgpDeviceStep block, then for every (struct type, address, final address)
        of ``rows`` that struct, or None when both addresses are 0."""
        io = FtgpDeviceStep(*(v or None for v in (stream, action, obs, reward, terminated, truncated, final_obs)))
        return [C.byref(io)] + [C.byref(T(a or None, b or None)) if a or b else None for T, a, b in rows]

    def step_device(self, action: int, obs: int, reward: int, terminated: int, truncated: int, final_obs: int = 0, stream: int = 0,
                    state: int = 0, final_state: int = 0, contact: int = 0, final_contact: int = 0):
        """One ftgp_step_device call on integer device addresses (and an integer hipStream_t, 0 = the null stream); only enqueues.
        With ``state`` or ``final_state``: ftgp_step_device_ex; with ``contact`` or ``final_contact``: ftgp_step_device_contacts."""
        io, extra, con = self._step_args(stream, action, obs, reward, terminated, truncated, final_obs,
                                         (FtgpDeviceStepExtra, state, final_state), (FtgpDeviceStepContacts, contact, final_contact))
        if con is not None:
            self._call("step_device_contacts", io, extra, con)
        elif extra is not None:
            self._call("step_device_ex", io, extra)
        else:
            self._call("step_device", io)

    def step_device_frame(self, action: int, obs: int, reward: int, terminated: int, truncated: int, final_obs: int = 0, stream: int = 0,
                          state: int = 0, final_state: int = 0, contact: int = 0, final_contact: int = 0, frame: int = 0,
                          final_frame: int = 0):
        """One ftgp_step_device_frame call on integer device addresses, like ``step_device``; ``frame`` / ``final_frame``: float32
        [n_envs, n_ext, FRAME_FIXED + 2 * n_ahead], either may be 0."""
        self._call("step_device_frame", *self._step_args(
            stream, action, obs, reward, terminated, truncated, final_obs, (FtgpDeviceStepExtra, state, final_state),
            (FtgpDeviceStepContacts, contact, final_contact), (FtgpDeviceStepFrame, frame, final_frame)))

    def step_device_rivals(self, action: int, obs: int, reward: int, terminated: int, truncated: int, final_obs: int = 0, stream: int = 0,
                           state: int = 0, final_state: int = 0, contact: int = 0, final_contact: int = 0, frame: int = 0,
                           final_frame: int = 0, rival: int = 0, final_rival: int = 0):
        """One ftgp_step_device_rivals call on integer device addresses, like ``step_device_frame``; ``rival`` / ``final_rival``:
        float32 [n_envs, n_ext, RIVAL_FIXED + RIVAL_FLOATS * n_rivals], either may be 0."""
        self._call("step_device_rivals", *self._step_args(
            stream, action, obs, reward, terminated, truncated, final_obs, (FtgpDeviceStepExtra, state, final_state),
            (FtgpDeviceStepContacts, contact, final_contact), (FtgpDeviceStepFrame, frame, final_frame),
            (FtgpDeviceStepRivals, rival, final_rival)))

    def state_device(self, state: int, stream: int = 0):
        """ftgp_state_device: the state rows of the current state into device memory at ``state``, ordered on ``stream``; only enqueues."""
        self._call("state_device", stream or None, state or None)

    def contacts_device(self, contact: int, stream: int = 0):
        """ftgp_contacts_device: the external cars' contact rows at the current state into device memory at ``contact``, ordered on
        ``stream``; only enqueues."""
        self._call("contacts_device", stream or None, contact or None)

    def frame_device(self, frame: int, stream: int = 0):
        """ftgp_frame_device: the external cars' frame rows at the current state into device memory at ``frame``, ordered on
        ``stream``; only enqueues."""
        self._call("frame_device", stream or None, frame or None)

    def rivals_device(self, rival: int, stream: int = 0):
        """ftgp_rivals_device: the external cars' rival rows at the current state into device memory at ``rival``, ordered on
        ``stream``; only enqueues."""
        self._call("rivals_device", stream or None, rival or None)

    # -- read-backs
    def get_rivals(self, n_rivals: int = 0) -> np.ndarray:
        """float32 [n_cars, RIVAL_FIXED + RIVAL_FLOATS * n_rivals] (RIVAL_FIELDS, then the mate slots of RIVAL_MATE_FIELDS): the rival
        row of every car at the current state (ftgp_get_rivals)."""
        n_rivals = int(n_rivals)
        if not 0 <= n_rivals <= MAX_RIVALS:
            raise ValueError(f"n_rivals: 0 .. {MAX_RIVALS}, got {n_rivals}")
        out = np.empty((self.n_cars, RIVAL_FIXED + RIVAL_FLOATS * n_rivals), dtype=np.float32)
        self._call("get_rivals", n_rivals, _ptr(out))
        return out

    def get_frames(self, n_ahead: int = 0, stride: int = 1) -> np.ndarray:
        """float32 [n_cars, FRAME_FIXED + 2 * n_ahead] (FRAME_FIELDS, then the look-ahead points): the frame row of every car at the
        current state (ftgp_get_frames)."""
        n_ahead = int(n_ahead)
        if not 0 <= n_ahead <= MAX_LOOKAHEAD:
            raise ValueError(f"n_ahead: 0 .. {MAX_LOOKAHEAD}, got {n_ahead}")
        out = np.empty((self.n_cars, FRAME_FIXED + 2 * n_ahead), dtype=np.float32)
        self._call("get_frames", n_ahead, int(stride), _ptr(out))
        return out

    def contacts(self) -> np.ndarray:
        """float32 [n_cars, 4] (CONTACT_FIELDS): the contact row of every car at the current state (ftgp_get_contacts)."""
        out = np.empty((self.n_cars, CONTACT_FLOATS), dtype=np.float32)
        self._call("get_contacts", _ptr(out))
        return out

    def lidar(self) -> np.ndarray:
        out = np.empty((self.n_cars, self.n_rays), dtype=np.float32)
        self._call("get_lidar", _ptr(out))
        return out

    def snapshot(self) -> np.ndarray:
        out = np.empty((self.n_cars, SNAPSHOT_DOUBLES), dtype=np.float64)
        self._call("get_snapshot", _ptr(out))
        return out

    def pose(self) -> np.ndarray:
        out = np.empty((self.n_cars, POSE_DOUBLES), dtype=np.float64)
        self._call("get_pose", _ptr(out))
        return out

    def set_pose(self, pose: np.ndarray):
        p = np.ascontiguousarray(pose, dtype=np.float64).reshape(self.n_cars, POSE_DOUBLES)
        self._call("set_pose", _ptr(p))

    def policy_eval(self, policy, ranges: np.ndarray) -> np.ndarray:
        p = POLICY_BY_NAME[policy] if isinstance(policy, str) else int(policy)
        r = np.ascontiguousarray(ranges, dtype=np.float32).reshape(self.n_cars, self.n_rays)
        out = np.empty((self.n_cars, 2), dtype=np.float64)
        self._call("policy_eval", p, _ptr(r), _ptr(out))
        return out

    def eval_progress(self):
        self._call("eval_progress")

    def progress(self) -> np.ndarray:
        out = np.empty((self.n_cars, PROGRESS_INTS), dtype=np.int32)
        self._call("get_progress", _ptr(out))
        return out

    def centre_dist2(self) -> np.ndarray:
        """float64 [n_cars]: the squared distance to the nearest centre-line point the progress block stored last (custom.py:1343)."""
        out = np.empty(self.n_cars, dtype=np.float64)
        self._call("get_centre_dist2", _ptr(out))
        return out

    def winners(self) -> np.ndarray:
        """Place of each car among the finishers of its env (1 = winner, 0 = still racing): Mujoco.winners, custom.py:1367-1369."""
        out = np.empty(self.n_cars, dtype=np.int32)
        self._call("get_winners", _ptr(out))
        return out.reshape(self.n_envs, self.cars_per_env)

    def lap_times(self):
        """(counts, ring): counts[i] = len(VehicleState.times) of car i (the true count), ring[i] = the ring of its newest
        MAX_LAP_TIMES lap times, lap time k in slot k % MAX_LAP_TIMES (see ``lap_time_list``)."""
        counts = np.empty(self.n_cars, dtype=np.int32)
        times = np.empty((self.n_cars, MAX_LAP_TIMES), dtype=np.float64)
        self._call("get_lap_times", _ptr(counts), _ptr(times))
        return counts, times

    def race_steps(self) -> np.ndarray:
        """int64 [n_cars, 2] = (start, finish_step): vehicle_state.start (custom.py:1362) and the step at which `finished` was set (-1 while
        racing), with all 64 bits of self.steps (columns 6 and 9 of ``progress()`` saturate at 2**31 - 1)."""
        out = np.empty((self.n_cars, 2), dtype=np.int64)
        self._call("get_race_steps", _ptr(out))
        return out

    def ctrl(self) -> np.ndarray:
        out = np.empty((self.n_cars, 2), dtype=np.float64)
        self._call("get_ctrl", _ptr(out))
        return out

    def steps(self) -> np.ndarray:
        out = np.empty(self.n_envs, dtype=np.int64)
        self._call("get_steps", _ptr(out))
        return out

    def metrics_local(self) -> np.ndarray:
        out = np.empty(METRIC_DOUBLES, dtype=np.float64)
        self._call("metrics_local", _ptr(out))
        return out

    # -- multi-GPU
    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        buf = np.frombuffer(unique_id, dtype=np.uint8).copy()
        assert buf.size == 128
        self.world_size = world_size
        self._call("comm_init", _ptr(buf), int(rank), int(world_size))

    def metrics_allgather(self) -> np.ndarray:
        out = np.empty((getattr(self, "world_size", 1), METRIC_DOUBLES), dtype=np.float64)
        self._call("metrics_allgather", _ptr(out))
        return out

    def metrics_allgather_begin(self):
        """Enqueue the exchange of the latest launch's record on the side stream and return at once."""
        self._call("metrics_allgather_begin")

    def metrics_allgather_end(self) -> np.ndarray:
        """Wait for the exchange begun last (not for any later launch) and return the [world, 8] records."""
        out = np.empty((getattr(self, "world_size", 1), METRIC_DOUBLES), dtype=np.float64)
        self._call("metrics_allgather_end", _ptr(out))
        return out

    def distance_field(self) -> np.ndarray:
        """FAKELIDAR mode: the Euclidean distance transform built at create, float64 [H, W] in pixels (self.dt of custom.py:1152-1153)."""
        out = np.empty((self.track.height, self.track.width), dtype=np.float64)
        self._call("get_distance_field", _ptr(out))
        return out

    def get_distance_field(self, track: int = 0) -> np.ndarray:
        """FAKELIDAR mode: the distance transform of track ``track`` of the handle, float64 [H, W] of that track, in pixels."""
        track = int(track)
        if not 0 <= track < len(self.tracks):
            raise ValueError(f"track {track} of a handle with {len(self.tracks)}")
        t = self.tracks[track]
        out = np.empty((t.height, t.width), dtype=np.float64)
        if len(self.tracks) == 1:
            self._call("get_distance_field", _ptr(out))
        else:
            self._call("get_track_distance_field", track, _ptr(out))
        return out

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._call("last_kernel_ms", C.byref(ms))
        return float(ms.value)

    def kernel_name(self) -> str:
        s = self.lib.fn("kernel_name")(self.h)
        return s.decode() if s else ""


# the car record of an env-state record (include/ftgp.h), 448 bytes
CAR_STATE_DTYPE = np.dtype(
    [(n, "<f8") for n in ("x", "y", "qw", "qz", "vx", "vy", "wz", "qs", "qsd")] + [("w", "<f8", (4,))]
    + [(n, "<f8") for n in ("u_speed", "u_steer", "last_steer", "dist2")]
    + [(n, "<i4") for n in ("completion", "laps", "offset", "n_times", "good_start", "finished", "off_track", "delta")]
    + [("start", "<i8"), ("finish_step", "<i8"), ("_pad", "V8"), ("times", "<f8", (MAX_LAP_TIMES,))])
CAR_STATE_FIELDS = tuple(n for n in CAR_STATE_DTYPE.names if n != "_pad")
ENV_STATE_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_rays", "<i4"), ("cars_per_env", "<i4"), ("lidar_mode", "<i4"),
                                   ("reserved", "<i4"), ("fingerprint", "<u8"), ("steps", "<i8"), ("episodes", "<i8")])
assert CAR_STATE_DTYPE.itemsize == 448 and ENV_STATE_HEADER_DTYPE.itemsize == 48


def env_state_layout(n_rays: int, cars_per_env: int) -> dict:
    """Byte offsets and sizes of one env-state record (include/ftgp.h: ftgp_save_envs_device): "header", "steps", "episodes", "cars",
    "dyn", "ranges" = where each part starts; "car_bytes", "dyn_bytes", "row_bytes" = the stride of a car inside the three per-car
    parts; "bytes" = bytes_per_env.  Every part starts on a 16-byte boundary and the size is a multiple of 16."""
    n_rays, c = int(n_rays), int(cars_per_env)
    if n_rays < 1 or not 1 <= c <= 8:
        raise ValueError(f"n_rays >= 1 and 1 <= cars_per_env <= 8, got {n_rays}, {c}")
    car_bytes, dyn_bytes, row_bytes = CAR_STATE_DTYPE.itemsize, 8 * DYN_RECORD, (4 * n_rays + 15) & ~15
    cars = ENV_STATE_HEADER_DTYPE.itemsize
    dyn = cars + c * car_bytes
    ranges = dyn + c * dyn_bytes
    return {"header": 0, "steps": 32, "episodes": 40, "cars": cars, "dyn": dyn, "ranges": ranges, "car_bytes": car_bytes,
            "dyn_bytes": dyn_bytes, "row_bytes": row_bytes, "bytes": ranges + c * row_bytes}


def unpack_env_state(buf, n_rays: int, cars_per_env: int) -> dict:
    """Decode env-state records: ``buf`` = uint8, one record or [n] records of ``env_state_layout(...)["bytes"]`` bytes.  Returns a dict
    of arrays with a leading axis of n: the header fields (ENV_STATE_HEADER_DTYPE: magic ... fingerprint, steps, episodes) [n]; the car
    fields by name (CAR_STATE_FIELDS) [n, cars_per_env, ...]; "dyn" float64 [n, cars_per_env, DYN_RECORD]; "ranges" float32
    [n, cars_per_env, n_rays]."""
    lay = env_state_layout(n_rays, cars_per_env)
    b = np.ascontiguousarray(buf, dtype=np.uint8)
    if b.size % lay["bytes"] or (b.ndim > 1 and b.shape[-1] != lay["bytes"]):
        raise ValueError(f"records of {lay['bytes']} bytes, got shape {b.shape}")
    b = b.reshape(-1, lay["bytes"])
    n, c = b.shape[0], int(cars_per_env)
    head = np.ascontiguousarray(b[:, :lay["cars"]]).view(ENV_STATE_HEADER_DTYPE).reshape(n)
    out = {name: head[name].copy() for name in ENV_STATE_HEADER_DTYPE.names}
    cars = np.ascontiguousarray(b[:, lay["cars"]:lay["dyn"]]).view(CAR_STATE_DTYPE).reshape(n, c)
    out.update({name: cars[name].copy() for name in CAR_STATE_FIELDS})
    out["dyn"] = np.ascontiguousarray(b[:, lay["dyn"]:lay["ranges"]]).view("<f8").reshape(n, c, DYN_RECORD)
    rows = np.ascontiguousarray(b[:, lay["ranges"]:]).view("<f4").reshape(n, c, lay["row_bytes"] // 4)
    out["ranges"] = rows[:, :, :int(n_rays)].copy()
    return out


def track_fingerprint(track) -> int:
    """The track fingerprint of an env-state record (include/ftgp.h): the splitmix64 fold over width, height, the bitmap words (bits
    beyond the width cleared) and the bit patterns of the 200 path doubles."""
    m = (1 << 64) - 1

    def splitmix64(z):
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    bits = np.ascontiguousarray(track.bits, dtype=np.uint32).copy()
    if track.width % 32:
        bits[:, track.width // 32] &= np.uint32((1 << (track.width % 32)) - 1)
    bits[:, (track.width + 31) // 32:] = 0
    path = np.ascontiguousarray(track.path, dtype=np.float64).reshape(-1).view(np.uint64)
    h = 0
    for v in [track.width, track.height] + bits.reshape(-1).tolist() + path.tolist():
        h = splitmix64(h ^ int(v))
    return h


def lap_time_list(count: int, ring: np.ndarray) -> list:
    """The tail of VehicleState.times (custom.py:124) that the ring still holds, oldest first: all ``count`` lap times while
    count <= MAX_LAP_TIMES, the newest MAX_LAP_TIMES after that."""
    count = int(count)
    first = max(0, count - MAX_LAP_TIMES)
    # (a slot that reads NaN holds no entry: a backward crossing popped the lap time that had overwritten it, see include/ftgp.h)
    return [float(ring[k % MAX_LAP_TIMES]) for k in range(first, count) if ring[k % MAX_LAP_TIMES] == ring[k % MAX_LAP_TIMES]]


def fakelidar(lib: CLib, dt: np.ndarray, origins: np.ndarray, cosines: np.ndarray, sines: np.ndarray, eps: float = 2.0,
              device_id: int = 0):
    """Batched ``ft_grandprix.raycast.fakelidar``: origins [n, 2] px, cosines / sines [n, R] -> (scan [n, R], points [n, R, 2])."""
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 2)
    c = np.ascontiguousarray(cosines, dtype=np.float64).reshape(len(o), -1)
    s = np.ascontiguousarray(sines, dtype=np.float64).reshape(len(o), -1)
    scan = np.empty_like(c)
    pts = np.empty(c.shape + (2,), dtype=np.float64)
    if lib.prefix == "ftgp_":
        lib.check(lib.fn("fakelidar")(device_id, _ptr(dt), dt.shape[0], dt.shape[1], len(o), _ptr(o), c.shape[1], _ptr(c), _ptr(s),
                                      float(eps), _ptr(scan), _ptr(pts)))
    else:   # the oracle exposes the single-origin form
        for k in range(len(o)):
            lib.check(lib.fn("fakelidar")(float(o[k, 0]), float(o[k, 1]), _ptr(dt), dt.shape[0], dt.shape[1], c.shape[1],
                                          c[k].ctypes.data_as(C.c_void_p), s[k].ctypes.data_as(C.c_void_p), float(eps),
                                          scan[k].ctypes.data_as(C.c_void_p), pts[k].ctypes.data_as(C.c_void_p)))
    return scan, pts


def selftest(lib: CLib, device_id: int = 0) -> int:
    """Mismatches of the device self-test (``ftgp_selftest``); 0 is the only acceptable answer."""
    n = C.c_int64(-1)
    lib.check(lib.fn("selftest")(device_id, C.byref(n)))
    return int(n.value)


def comm_unique_id(lib: CLib) -> bytes:
    buf = np.zeros(128, dtype=np.uint8)
    lib.check(lib.fn("comm_unique_id")(_ptr(buf)))
    return buf.tobytes()
