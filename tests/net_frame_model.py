"""The network driver with frame inputs (include/ftgp.h: ftgp_set_net_frame), from the two models of the header's text: the input
vector is tests/net_model.py's inputs followed by tests/frame_model.py's frame row with the slot's own n_ahead and stride, then
net_model.forward.  Nothing here is taken from the kernels or from csrc/ftgp_frame.h.

A network is net_model's dict with three more keys: frame, lookahead, lookahead_stride.
"""
import numpy as np

from tests import frame_model as fm
from tests import net_model as nm

F = np.float32


def n_frame(net):
    return fm.FRAME_FIXED + 2 * net.get("lookahead", 0) if net.get("frame") else 0


def n_in(net):
    return net["n_beams"] + (5 if net.get("use_state") else 0) + n_frame(net)


def inputs(net, ranges, pose, ctrl, path):
    """float32 [n_cars, n_in]: beams, state entries 0 - 4, frame row.  `path` [100, 2], or one per car (a multi-track handle)."""
    x = [nm.beams(ranges, net["pool"], net["max_range"], net["beam_first"], net["n_beams"])]
    if net.get("use_state"):
        x.append(nm.state_inputs(pose, ctrl))
    if net.get("frame"):
        pose = np.asarray(pose, dtype=np.float64)
        if isinstance(path, (list, tuple)):
            rows = np.concatenate([fm.frame_rows(p, pose[i:i + 1], net.get("lookahead", 0), net.get("lookahead_stride", 1)) for i, p in enumerate(path)])
        else:
            rows = fm.frame_rows(path, pose, net.get("lookahead", 0), net.get("lookahead_stride", 1))
        x.append(rows)
    return np.concatenate(x, axis=1).astype(F)


def evaluate(net, ranges, pose, ctrl, path, finished=None):
    """(controls float64 [n_cars, 2], inputs float32 [n_cars, n_in])."""
    x = inputs(net, ranges, pose, ctrl, path)
    return nm.evaluate(net, None, finished=finished, inputs=x), x


def random_net(rng, hidden, *, n_beams, use_state=True, frame=True, lookahead=0, lookahead_stride=1, **kw):
    """net_model.random_net of widths (n_in, *hidden, 2) with the frame keys."""
    width0 = n_beams + (5 if use_state else 0) + (fm.FRAME_FIXED + 2 * lookahead if (frame or lookahead) else 0)
    net = nm.random_net(rng, (width0, *hidden, 2), use_state=use_state, **kw)
    net.update(n_beams=n_beams, frame=bool(frame or lookahead), lookahead=lookahead, lookahead_stride=lookahead_stride)
    return net


def fields(net):
    return {k: v for k, v in net.items() if k != "layers"}


def flat_params(net):
    return np.concatenate([np.concatenate([W.ravel(), b.ravel()]) for W, b in net["layers"]]).astype(F)


# ---------------------------------------------------------------------------------------------------------------------- poses
def yawed(x, y, yaw):
    """A row of ftgp_get_pose at (x, y) with heading yaw, at rest."""
    p = np.zeros(13)
    p[0], p[1], p[3], p[6] = x, y, np.cos(yaw / 2), np.sin(yaw / 2)
    return p


def pose_list(path, which):
    """The poses of the issue on `path` (`which`: "square", "dup" = the square with point 11 on point 10, "skew"): on a path point; on
    the outside of a bend where g2_A = g2_B; strictly inside a bend (A taken); nearest to point 0 from behind (A = 99 -> 0) and to
    point 99; nearest to a point of index >= 64; on the duplicated point (L2 == 0); far off the track."""
    P = np.asarray(path, dtype=np.float64)
    poses = [
        yawed(P[5, 0], P[5, 1], 0.3),                                  # on a path point
        yawed(P[25, 0] + 0.5, P[25, 1] - 0.5, 1.1),                    # outside the bend at point 25: both segments clamp to it, g2_A = g2_B
        yawed(P[25, 0] - 0.125, P[25, 1] + 0.0625, 2.0),               # strictly inside that bend, nearer to segment A = 24 -> 25
        yawed(P[0, 0] + 0.0625, P[0, 1] + 0.125, -1.3),                # nearest to point 0, nearer to A = 99 -> 0 than to B
        yawed(P[99, 0] + 0.03125, P[99, 1] + 0.0625, 2.9),             # nearest to point 99
        yawed(P[70, 0] - 0.2, P[70, 1] + 0.3, -2.2),                   # c >= 64: the second point of a lane
        yawed(P[88, 0] + 0.1, P[88, 1] - 0.05, 0.0),
        yawed(P[10, 0], P[10, 1], 0.7),                                # on the duplicated point (where the path has one)
        yawed(P[10, 0] + 0.1, P[10, 1] + 0.2, -0.4),                   # ... and beside it
        yawed(P[50, 0] + 9.0, P[50, 1] + 7.0, 0.9),                    # far off the track
    ]
    if which == "skew":
        poses.append(yawed(fm.SKEW_WRAP_POSE[0], fm.SKEW_WRAP_POSE[1], 0.2))      # a = 99 with t = 1: s = 100 wraps to 0
    poses = np.stack(poses)
    poses[:, 7:9] = np.random.default_rng(5).uniform(-3, 3, (len(poses), 2))      # velocities for the state inputs
    poses[:, 12] = np.linspace(-2, 2, len(poses))
    return poses


def paths():
    return {"square": fm.square_path(), "dup": fm.square_path(duplicate=10), "skew": fm.skew_path()}
