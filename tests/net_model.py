"""The network driver of include/ftgp.h ("Network drivers"), restated in numpy from the header's text -- not from csrc/ftgp_net.h.

Everything is binary32 with one rounding per written operation; fmaf is EXACT: the product of two binary32 numbers is exact in
binary64 (48 bits), the sum with the addend is taken with a two-sum, the binary64 sum is nudged to odd where the error is not zero
(round to odd keeps 53 >= 2 * 24 + 2 bits, so the second rounding to binary32 is the rounding of the exact value), then rounded.
Vectorised over cars: a network of 256 inputs is a few hundred numpy calls.
"""
import numpy as np

F = np.float32
ACT = {"identity": 0, "relu": 1, "tanh": 2}


def fmaf(a, b, c):
    """float32 fma(a, b, c) with one rounding, element-wise (arrays broadcast)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=F), np.asarray(b, dtype=F), np.asarray(c, dtype=F))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)            # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                          # exact: s + err = p + c
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        nudge = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((bits & 1) == 0)
        toward = np.where(err > 0.0, np.inf, -np.inf)
        s = np.where(nudge, np.nextafter(s, toward), s)
        return s.astype(F)


def clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v): a NaN stays a NaN."""
    v = np.asarray(v, dtype=F)
    return np.where(v < F(lo), F(lo), np.where(v > F(hi), F(hi), v)).astype(F)


def tanh(acc):
    """Lambert's continued fraction, twelve levels, from the inside out."""
    with np.errstate(all="ignore"):
        x = clamp(acc, -9.0, 9.0)
        x2 = (x * x).astype(F)
        d = np.full_like(x2, F(25.0))
        for k in range(11, -1, -1):
            d = (F(2 * k + 1) + (x2 / d).astype(F)).astype(F)
        return clamp((x / d).astype(F), -1.0, 1.0)


def relu(acc):
    acc = np.asarray(acc, dtype=F)
    return np.where(acc > F(0.0), acc, F(0.0)).astype(F)


def act(name, acc):
    return tanh(acc) if name == "tanh" else relu(acc) if name == "relu" else np.asarray(acc, dtype=F)


def beams(ranges, pool, max_range, beam_first, n_beams):
    """float32 [n_cars, n_beams]: s(r) = r < 0 ? M : (r < M ? r : M); the minimum in ray order, the first of equals stays; times
    float32(1) / float32(M)."""
    r = np.asarray(ranges, dtype=F)
    M = F(max_range)
    inv = F(F(1.0) / M)
    r = r[:, beam_first * pool:(beam_first + n_beams) * pool].reshape(r.shape[0], n_beams, pool)
    s = np.where(r < F(0.0), M, np.where(r < M, r, M)).astype(F)
    m = s[:, :, 0]
    for p in range(1, pool):
        m = np.where(s[:, :, p] < m, s[:, :, p], m)
    return (m * inv).astype(F)


def state_inputs(pose, ctrl):
    """float32 [n_cars, 5] from ftgp_get_pose rows (x y z qw qx qy qz vx vy vz wx wy wz) and ftgp_get_ctrl rows: entries 0 - 4 of the
    state row, binary64 with one rounding per operation, each rounded once to binary32."""
    pose, ctrl = np.asarray(pose, dtype=np.float64), np.asarray(ctrl, dtype=np.float64)
    qw, qz, vx, vy, wz = pose[:, 3], pose[:, 6], pose[:, 7], pose[:, 8], pose[:, 12]
    c = qw * qw - qz * qz
    s = 2.0 * (qw * qz)
    return np.stack([vx * c + vy * s, vy * c - vx * s, wz, ctrl[:, 0], ctrl[:, 1]], axis=1).astype(F)


def forward(x, layers, hidden_act, out_act):
    """The layers on inputs x float32 [n_cars, n_in]: acc = b[j]; acc = fmaf(W[j][k], x[k], acc) for k ascending; the activation."""
    x = np.asarray(x, dtype=F)
    for l, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=F), np.asarray(b, dtype=F)
        acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[0])).astype(F)
        for k in range(W.shape[1]):
            acc = fmaf(W[None, :, k], x[:, k, None], acc)
        x = act(hidden_act if l + 1 < len(layers) else out_act, acc)
    return x


def controls(y, out_scale, out_offset, finished=None):
    """float64 [n_cars, 2]: fmaf(y, scale, offset) widened; a car with a non-finite one gets (0, 0); a finished car gets (0, 0)."""
    u = fmaf(y[:, :2], np.asarray(out_scale, dtype=F)[None, :], np.asarray(out_offset, dtype=F)[None, :]).astype(np.float64)
    ok = np.isfinite(u).all(axis=1)
    if finished is not None:
        ok &= ~np.asarray(finished, dtype=bool)
    return np.where(ok[:, None], u, 0.0)


def evaluate(net, ranges, pose=None, ctrl=None, finished=None, inputs=None):
    """The controls of every car for `net` = dict(layers, pool, max_range, beam_first, n_beams, use_state, hidden_act, out_act,
    out_scale, out_offset) on full scans `ranges` [n_cars, n_rays] -- or on `inputs` [n_cars, n_in] given outright."""
    if inputs is None:
        x = beams(ranges, net["pool"], net["max_range"], net["beam_first"], net["n_beams"])
        if net.get("use_state"):
            x = np.concatenate([x, state_inputs(pose, ctrl)], axis=1)
    else:
        x = np.asarray(inputs, dtype=F)
    y = forward(x, net["layers"], net.get("hidden_act", "tanh"), net.get("out_act", "tanh"))
    return controls(y, net.get("out_scale", (1, 1)), net.get("out_offset", (0, 0)), finished)


def random_net(rng, widths, *, pool, max_range, beam_first, use_state=False, hidden_act="tanh", out_act="tanh", out_scale=(1, 1),
               out_offset=(0, 0), gain=1.0):
    """A random network of the given widths (n_in, ..., 2): weights ~ N(0, gain / sqrt(n_in)), biases ~ N(0, 0.1)."""
    layers = []
    for n_in, n_out in zip(widths[:-1], widths[1:]):
        layers.append(((rng.standard_normal((n_out, n_in)) * gain / np.sqrt(n_in)).astype(F), (0.1 * rng.standard_normal(n_out)).astype(F)))
    return dict(layers=layers, pool=pool, max_range=max_range, beam_first=beam_first, n_beams=widths[0] - (5 if use_state else 0),
                use_state=use_state, hidden_act=hidden_act, out_act=out_act, out_scale=out_scale, out_offset=out_offset)


# The shapes of the policy_eval scenarios and of the host-harness pin: name -> (n_rays, the four networks of slots 0 .. 3).
def eval_cases(seed=11):
    rng = np.random.default_rng(seed)
    r = lambda widths, **kw: random_net(rng, widths, **kw)         # noqa: E731
    small = dict(pool=4, max_range=3.0, beam_first=2)
    wide = dict(pool=10, max_range=10.0, beam_first=14, use_state=True)
    limit = dict(pool=4, max_range=8.0, beam_first=42, use_state=True)
    one = dict(pool=1, max_range=2.5, beam_first=8)
    return {
        "one_layer": (64, [r((12, 2), hidden_act="identity", out_act="identity", out_scale=(s, 1.0), out_offset=(0.5, -s), **small) for s in (1.0, 2.0, 0.5, 3.0)]),
        "mlp_tanh": (1080, [r((85, 64, 64, 2), out_scale=(3.5, 0.6), out_offset=(3.5, 0.0), gain=g, **wide) for g in (1.0, 2.0, 4.0, 0.5)]),
        "off_wave": (1080, [r((85, 37, 2), hidden_act="relu", out_act=a, **wide) for a in ("identity", "relu", "tanh", "identity")]),
        "limits": (1344, [r((256, 128, 128, 128, 2), hidden_act=h, gain=2.0, **limit) for h in ("tanh", "relu", "tanh", "identity")]),
        "pool_one": (64, [r((48, 16, 2), hidden_act=h, out_act="identity", **one) for h in ("tanh", "relu", "identity", "tanh")]),
    }


def eval_scans(rng, n_cars, n_rays, max_range):
    """Scans with -1 (no hit), 0, values above M and values equal to M among ordinary ranges."""
    M = F(max_range)
    s = rng.uniform(0.05, 1.3 * float(M), (n_cars, n_rays)).astype(F)
    pick = rng.integers(0, 12, s.shape)
    s[pick == 0] = F(-1.0)
    s[pick == 1] = F(0.0)
    s[pick == 2] = M
    s[pick == 3] = F(2.0) * M
    return s


def eval_records(rng, n_cars):
    """(pose rows, ctrl rows) with random planar velocities, headings and controls."""
    pose = np.zeros((n_cars, 13))
    yaw = rng.uniform(-np.pi, np.pi, n_cars)
    pose[:, 3], pose[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    pose[:, 7:9] = rng.uniform(-4, 4, (n_cars, 2))
    pose[:, 12] = rng.uniform(-3, 3, n_cars)
    return pose, np.stack([rng.uniform(0, 7, n_cars), rng.uniform(-1, 1, n_cars)], axis=1)
