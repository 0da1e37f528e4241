"""The network driver with rival inputs (include/ftgp.h: ftgp_set_net_rivals), from the models of the header's text: the input vector
is tests/net_frame_model.py's (beams, state entries, frame row) followed by tests/rival_model.py's rival row of the car's env with the
slot's own n_rivals, then net_model.forward.  Nothing here is taken from the kernels or from csrc/ftgp_rival.h.

A network is net_frame_model's dict with two more keys: rivals, n_rivals.  The records of an env are a dict `race`: abs_completion
(column 3 of ftgp_get_progress), finished (column 4), finish_step (column 1 of ftgp_get_race_steps), and cpe = cars per env; the cars
are those of whole envs, one env after the other.
"""
import numpy as np

from tests import frame_model as fm
from tests import net_frame_model as nfm
from tests import net_model as nm
from tests import rival_model as rm

F = np.float32


def n_rival(net):
    return rm.RIVAL_FIXED + rm.RIVAL_FLOATS * net.get("n_rivals", 0) if net.get("rivals") else 0


def n_in(net):
    return nfm.n_in(net) + n_rival(net)


def race_of(env, cpe=None):
    """The race records of a handle (capi.Env) as the model takes them."""
    prog, rs = env.progress(), env.race_steps()
    return dict(abs_completion=prog[:, 3].copy(), finished=prog[:, 4].copy(), finish_step=rs[:, 1].copy(), cpe=cpe or env.n_cars // env.n_envs)


def rival_block(net, pose, race, path):
    """float32 [n_cars, 4 + 8 n_rivals]: every car's rival row.  `path` [100, 2], or one per car (a multi-track handle: the cars of an
    env share theirs)."""
    cpe, n = race["cpe"], len(pose)
    pose = np.asarray(pose, dtype=np.float64)
    if isinstance(path, (list, tuple)):
        out = []
        for e0 in range(0, n, cpe):
            k = slice(e0, e0 + cpe)
            out.append(rm.rival_rows(path[e0], pose[k], race["abs_completion"][k], race["finished"][k], race["finish_step"][k], cpe, net["n_rivals"]))
        return np.concatenate(out)
    return rm.rival_rows(path, pose, race["abs_completion"], race["finished"], race["finish_step"], cpe, net["n_rivals"])


def inputs(net, ranges, pose, ctrl, path, race):
    """float32 [n_cars, n_in] of ALL cars of the envs: beams, state entries 0 - 4, frame row, rival row."""
    x = nfm.inputs(net, ranges, pose, ctrl, path)
    if net.get("rivals"):
        x = np.concatenate([x, rival_block(net, pose, race, path)], axis=1)
    return x.astype(F)


def evaluate(net, ranges, pose, ctrl, path, race, finished=None):
    """(controls float64 [n_cars, 2], inputs float32 [n_cars, n_in]); finished: who gets (0, 0) before the network is looked at."""
    x = inputs(net, ranges, pose, ctrl, path, race)
    return nm.evaluate(net, None, finished=finished, inputs=x), x


def random_net(rng, hidden, *, n_beams, use_state=True, frame=False, lookahead=0, lookahead_stride=1, rivals=True, n_rivals=0, **kw):
    """net_model.random_net of widths (n_in, *hidden, 2) with the frame keys and the rival keys."""
    on = bool(rivals or n_rivals)
    width0 = n_beams + (5 if use_state else 0) + (fm.FRAME_FIXED + 2 * lookahead if (frame or lookahead) else 0) + (rm.RIVAL_FIXED + rm.RIVAL_FLOATS * n_rivals if on else 0)
    net = nm.random_net(rng, (width0, *hidden, 2), use_state=use_state, **kw)
    net.update(n_beams=n_beams, frame=bool(frame or lookahead), lookahead=lookahead, lookahead_stride=lookahead_stride, rivals=on, n_rivals=n_rivals)
    return net


def identity_net(n_beams, n_rivals, pick=(0, 1), **kw):
    """One identity layer whose two outputs are inputs pick[0] and pick[1] as they are (weights 1.0, bias 0): the controls show two
    entries of the vector themselves."""
    net = random_net(np.random.default_rng(0), (), n_beams=n_beams, n_rivals=n_rivals, hidden_act="identity", out_act="identity", **kw)
    W = np.zeros_like(net["layers"][0][0])
    W[0, pick[0]], W[1, pick[1]] = 1.0, 1.0
    net["layers"] = [(W, np.zeros(2, dtype=F))]
    return net


fields = nfm.fields
flat_params = nfm.flat_params


# ---------------------------------------------------------------------------------------------------------------------- envs
def scene_env(cars, shift=(0.0, 0.0)):
    """(pose, race) of one of rival_model.hand_scenes()'s envs, moved by `shift`."""
    pose, ac, fin, fs = rm.scene_arrays(cars)
    pose[:, 0] += shift[0]; pose[:, 1] += shift[1]
    return pose, dict(abs_completion=ac, finished=fin, finish_step=fs, cpe=len(cars))


def extra_scenes():
    """Envs on frame_model.square_path() beyond rival_model.hand_scenes(), in its format: finishers with different finish steps and a
    finished car `a` among racing ones; track_gap and f_b at the wrap (s_b - s_a = +-50 exactly; s - c = 50 cannot happen, |s - c| <= 1,
    so f_b wraps where c = 0 and s = 99.5); a mate with the larger slot but the larger g."""
    E = rm.EAST
    return {
        "finishers, different steps": [(3.25, 0.0, E, 0.0, 0.0, 6, 0, 0), (4.25, 0.0, E, 0.0, 0.0, 100, 1, 120), (6.25, 0.0, E, 0.0, 0.0, 100, 1, 95),
                                       (2.25, 0.0, E, 1.0, 0.0, 4, 0, 0)],
        "finishers, steps past 2^32": [(4.25, 0.0, E, 0.0, 0.0, 100, 1, (1 << 32) + 5), (6.25, 0.0, E, 0.0, 0.0, 100, 1, 7), (2.25, 0.0, E, 1.0, 0.0, 4, 0, 0)],
        "everyone finished": [(4.25, 0.0, E, 0.0, 0.0, 100, 1, 50), (6.25, 0.0, E, 0.0, 0.0, 100, 1, 50)],
        "track_gap +50 and -50": [(2.5, 0.0, E, 0.0, 0.0, 5, 0, 0), (10.0, 12.5, E, 0.0, 0.0, 55, 0, 0)],
        "f wraps: c = 0, s = 99.5": [(0.0, 0.25, E, 0.0, 0.0, 100, 0, 0), (0.25, 0.0, E, 0.0, 0.0, 100, 0, 0), (0.0, 0.75, E, 0.0, 0.0, 99, 0, 0)],
    }


def all_scenes():
    return {**rm.hand_scenes(), **extra_scenes()}


def random_env(path, rng, cpe, finished=0):
    """cpe cars near `path` in rival_model.hand_scenes()'s format, the first `finished` of a random order finished."""
    cars = []
    who = set(rng.permutation(cpe)[:finished].tolist())
    for k in range(cpe):
        i, w = int(rng.integers(100)), rng.uniform()
        p = (1 - w) * path[i] + w * path[(i + 1) % 100] + rng.uniform(-0.9, 0.9, 2)
        yaw = rng.uniform(-np.pi, np.pi)
        fin = int(k in who)
        cars.append((p[0], p[1], (np.cos(yaw / 2), np.sin(yaw / 2)), *rng.uniform(-4.0, 4.0, 2), 100 if fin else int(rng.integers(-20, 90)), fin,
                     int(rng.integers(50, 54)) if fin else 0))
    return cars
