"""Training on the device (include/ftgp.h "Training on the device"), restated in numpy from the header's text -- not from csrc/ftgp_net.h
or the kernels.  The forward pass to the bit is tests/net_model.py; here are the loss, its gradient by hand (the calculus the kernel
must reproduce), the stats and Adam's element step.

loss_and_grad(case, dtype): binary64 is the reference (np.tanh: the derivative 1 - o*o is then exact calculus); binary32 is "the same
model in binary32" -- the specified TANH, numpy's float32 products, the batch rows accumulated one after the other -- whose distance from
the reference sets the tolerance of the device (tests/test_train.py).

CASES: the gradient cases (a - e, turns32 / turns16, mixed / mixed2, edge32 / edge16, uneven); row_layout restates how the host cuts an LDS row and
chooses 32 or 16 rows a tile, from ftgp_train_grad_device's text; turns_rows / turns_index build the batches of the `turns` scenario.
"""
import numpy as np

from tests import net_model as nm

F = np.float32
STATS = 8


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_scalars(beta1, beta2, lr, t):
    """(b1, b2, omb1, omb2, a, r) as binary32: binary64, each rounded once."""
    b1, b2 = float(F(beta1)), float(F(beta2))
    return (F(beta1), F(beta2), F(1.0 - b1), F(1.0 - b2), F(float(F(lr)) / (1.0 - b1 ** float(t))), F(1.0 / np.sqrt(1.0 - b2 ** float(t))))


def adam_step(p, m, v, g, scalars, eps):
    """One step on float32 arrays: m = fmaf(b1, m, omb1*g); v = fmaf(b2, v, omb2*(g*g)); d = fmaf(sqrtf(v), r, eps); p = fmaf(-a, m/d, p)."""
    b1, b2, omb1, omb2, a, r = scalars
    p, m, v, g = (np.asarray(x, dtype=F) for x in (p, m, v, g))
    with np.errstate(all="ignore"):
        m1 = nm.fmaf(b1, m, (omb1 * g).astype(F))
        v1 = nm.fmaf(b2, v, (omb2 * (g * g).astype(F)).astype(F))
        d = nm.fmaf(np.sqrt(v1).astype(F), r, F(eps))
        p1 = nm.fmaf(F(-a), (m1 / d).astype(F), p)
    return p1, m1, v1


def flat(layers):
    """torch's nn.Linear layout in one flat buffer: per layer W[n_out][n_in], then b[n_out]."""
    return np.concatenate([np.concatenate([np.asarray(W, dtype=F).ravel(), np.asarray(b, dtype=F).ravel()]) for W, b in layers])


def unflat(buf, widths):
    out, at = [], 0
    for n_in, n_out in zip(widths[:-1], widths[1:]):
        W = buf[at:at + n_out * n_in].reshape(n_out, n_in); at += n_out * n_in
        b = buf[at:at + n_out]; at += n_out
        out.append((W, b))
    assert at == buf.size
    return out


# ------------------------------------------------------------------------------------------------------------------ the loss and its gradient
def _act(name, a, dtype):
    if name == "tanh":
        return np.tanh(a) if dtype == np.float64 else nm.tanh(a)
    if name == "relu":
        return np.where(a > 0, a, 0).astype(dtype)
    return a


def _slope(name, o):
    return 1 - o * o if name == "tanh" else (o > 0).astype(o.dtype) if name == "relu" else np.ones_like(o)


def _forward(x, net, dtype):
    """The stored outputs of every layer (outs[0] = x) and the pre-activations."""
    outs, pre = [x.astype(dtype)], []
    n = len(net["layers"])
    for l, (W, b) in enumerate(net["layers"]):
        a = (outs[-1] @ np.asarray(W, dtype=dtype).T + np.asarray(b, dtype=dtype)).astype(dtype)
        pre.append(a)
        outs.append(_act(net["hidden_act"] if l + 1 < n else net["out_act"], a, dtype).astype(dtype))
    return outs, pre


def _backward(net, outs, delta, dtype, by_row):
    """[(dW, db)] from the delta at the last layer's pre-activation; by_row: the rows accumulated one after the other."""
    grads = [None] * len(net["layers"])
    for l in range(len(net["layers"]) - 1, -1, -1):
        x = outs[l]
        if by_row:
            dW, db = np.zeros((delta.shape[1], x.shape[1]), dtype=dtype), np.zeros(delta.shape[1], dtype=dtype)
            for r in range(x.shape[0]):
                dW = (dW + np.outer(delta[r], x[r]).astype(dtype)).astype(dtype)
                db = (db + delta[r]).astype(dtype)
        else:
            dW, db = delta.T @ x, delta.sum(axis=0)
        grads[l] = (dW.astype(dtype), db.astype(dtype))
        if l > 0:
            delta = ((delta @ np.asarray(net["layers"][l][0], dtype=dtype)) * _slope(net["hidden_act"], outs[l])).astype(dtype)
    return grads


def loss_terms(case, dtype=np.float64, layers=None):
    """Per-row quantities and the two sums of L for the batch rows of `case` (see make_case), in `dtype`."""
    pol, val = dict(case["policy"]), dict(case["value"])
    if layers is not None:
        pol["layers"], val["layers"] = layers
    rows = case["rows"]
    x = case["inputs"][rows]
    w = (case["weight"][rows] if case["weight"] is not None else np.ones(len(rows))).astype(dtype)
    noise = (case["noise"][rows] if case["noise"] is not None else np.zeros((len(rows), 2))).astype(dtype)
    mean, A, ret = case["mean"][rows].astype(dtype), case["advantage"][rows].astype(dtype), case["ret"][rows].astype(dtype)
    std, c, coef = np.asarray(case["std"], dtype=dtype), dtype(case["clip"]), dtype(case["value_coef"])
    po, ppre = _forward(x, pol, dtype)
    vo, vpre = _forward(x, val, dtype)
    m = (po[-1] * np.asarray(pol["out_scale"], dtype=dtype) + np.asarray(pol["out_offset"], dtype=dtype)).astype(dtype)
    v = (vo[-1][:, 0] * dtype(val["out_scale"]) + dtype(val["out_offset"])).astype(dtype)
    p = (std * noise + mean).astype(dtype)
    z = ((p - m) / std).astype(dtype)
    logp, logq = (-0.5 * (z * z).sum(axis=1)).astype(dtype), (-0.5 * (noise * noise).sum(axis=1)).astype(dtype)
    rho = np.exp(logp - logq).astype(dtype)
    s = np.minimum(rho * A, np.clip(rho, 1 - c, 1 + c) * A).astype(dtype)
    active = ((A >= 0) & (rho <= 1 + c)) | ((A < 0) & (rho >= 1 - c))
    S = w.sum(dtype=dtype)
    return dict(pol=pol, val=val, po=po, vo=vo, ppre=ppre, vpre=vpre, m=m, v=v, z=z, logp=logp, logq=logq, rho=rho, s=s, active=active,
                w=w, A=A, ret=ret, std=std, c=c, coef=coef, S=S)


def loss(case, layers=None):
    """L in binary64 at the given (policy layers, value layers)."""
    t = loss_terms(case, np.float64, layers)
    return float(-(t["w"] * t["s"]).sum() / t["S"] + t["coef"] * (t["w"] * 0.5 * (t["v"] - t["ret"]) ** 2).sum() / t["S"])


def loss_and_grad(case, dtype=np.float64):
    """(policy grads [(dW, db)], value grads, stats float[8] without [5] and [6]) by the chain rule written out."""
    t = loss_terms(case, dtype)
    by_row = dtype != np.float64
    w, S = t["w"], t["S"]
    stats = np.zeros(STATS, dtype=dtype)
    if not S > 0:
        zero = lambda net: [(np.zeros_like(W, dtype=dtype), np.zeros_like(b, dtype=dtype)) for W, b in net["layers"]]   # noqa: E731
        return zero(t["pol"]), zero(t["val"]), stats
    up = np.where(t["active"], -(w * t["A"] * t["rho"]), 0).astype(dtype) / S                      # dL/drho ... times rho: dL/dlogp
    dm = (up[:, None] * (t["z"] / t["std"])).astype(dtype)                                         # dlogp/dm_k = z_k / std_k
    dpol = (dm * np.asarray(t["pol"]["out_scale"], dtype=dtype) * _slope(t["pol"]["out_act"], t["po"][-1])).astype(dtype)
    dv = (t["coef"] * w * (t["v"] - t["ret"]) / S).astype(dtype)
    dval = (dv * dtype(t["val"]["out_scale"]))[:, None] * _slope(t["val"]["out_act"], t["vo"][-1])
    gp = _backward(t["pol"], t["po"], dpol.astype(dtype), dtype, by_row)
    gv = _backward(t["val"], t["vo"], dval.astype(dtype), dtype, by_row)
    stats[0] = S
    stats[1] = -(w * t["s"]).sum(dtype=dtype) / S
    stats[2] = (w * (0.5 * (t["v"] - t["ret"]) ** 2)).sum(dtype=dtype) / S
    stats[3] = (w * (t["logq"] - t["logp"])).sum(dtype=dtype) / S
    stats[4] = (w * (np.abs(t["rho"] - 1) > t["c"])).sum(dtype=dtype) / S
    return gp, gv, stats


def conditions(case, high_side=True):
    """What a gradient case must offer, from the binary64 model: the clip binds on both sides and leaves rows free, no row sits at the
    clip's edge, no relu pre-activation at 0.  A string that names the first miss, or None.
    high_side=False is for a case without noise alone: there logq = 0 and rho = exp(logp) <= 1, so no ratio can pass 1 + clip, whatever
    the seed; the clip is then asked to bind on the low side only, and every ratio is asserted to be <= 1."""
    t = loss_terms(case, np.float64)
    w, S = t["w"], t["S"]
    off_hi = (w * (~t["active"] & (t["A"] >= 0))).sum() / S
    off_lo = (w * (~t["active"] & (t["A"] < 0))).sum() / S
    on = (w * t["active"]).sum() / S
    if not high_side:
        assert case["noise"] is None and (t["rho"] <= 1).all() and off_hi == 0
    if (high_side and off_hi < 0.05) or off_lo < 0.05:
        return f"the clip binds on {off_hi:.3f} / {off_lo:.3f} of the weighted rows"
    if on < 0.40:
        return f"only {on:.3f} of the weighted rows are free"
    for edge in (1 - t["c"], 1 + t["c"]):
        if (np.abs(t["rho"] - edge) <= 1e-4 * edge).any():
            return "a row's ratio sits at the clip's edge"
    for net, pre in ((t["pol"], t["ppre"]), (t["val"], t["vpre"])):
        for l, a in enumerate(pre):
            name = net["hidden_act"] if l + 1 < len(pre) else net["out_act"]
            if name == "relu" and (np.abs(a) <= 1e-5).any():
                return "a relu pre-activation sits at 0"
    return None


# ------------------------------------------------------------------------------------------------------------------ cases
def random_layers(rng, widths, gain=1.0):
    return [((rng.standard_normal((o, i)) * gain / np.sqrt(i)).astype(F), (0.1 * rng.standard_normal(o)).astype(F)) for i, o in zip(widths[:-1], widths[1:])]


# name -> (n_in, policy hidden widths, value hidden widths, hidden_act, policy out_act, n_rows, B, how the batch rows are chosen)
CASES = {
    "a": (85, (64, 64), (64, 64), "tanh", "tanh", 400, 517, "index"),
    "b": (1, (3,), (3,), "relu", "identity", 80, 63, "contiguous"),
    "c": (256, (128, 128, 128), (128, 128, 128), "tanh", "tanh", 330, 300, "contiguous"),
    "d": (33, (65,), (65,), "tanh", "tanh", 300, 257, "contiguous"),
    "e1": (33, (), (), "tanh", "tanh", 40, 1, "contiguous"),
    "e64": (33, (), (), "tanh", "tanh", 90, 64, "contiguous"),
    # more tiles than workgroups (258 tiles of 32 and of 16 rows, the last one ragged): workgroups 0 and 1 take a second tile
    "turns32": (17, (8,), (8,), "tanh", "tanh", 700, 8229, "index"),
    "turns16": (256, (128,), (128,), "tanh", "tanh", 500, 4115, "index"),
    # the two nets differ in depth and width; widths that are no multiple of 8 below the last layer; a bias row inside a 32-row tile of k
    "mixed": (33, (31, 97), (64,), "relu", "tanh", 300, 130, "contiguous"),
    "mixed2": (33, (), (100, 7, 33), "tanh", "identity", 300, 97, "contiguous"),
    # the two sides of the tile-size rule: an LDS row of 500 floats (32 rows: 64000 bytes) and of 508 (16 rows)
    "edge32": (104, (65, 65), (65, 65), "tanh", "tanh", 200, 70, "contiguous"),
    "edge16": (108, (65, 65), (65, 65), "tanh", "tanh", 200, 70, "contiguous"),
    # the middle layer 80 -> 24 has 3 x 2 tiles of the weight gradient for four waves: two waves reach the input delta, whose 128 columns
    # fill a whole delta buffer, while the other two still read the delta in hand -- the two buffers must not share a float
    "uneven": (33, (80, 24), (80, 24), "tanh", "tanh", 300, 70, "contiguous"),
}
LOOSE = ("e1",)      # one row cannot bind the clip on both sides: the conditions are not asked of it
MAX_WG = 256         # FTGP_TRAIN_MAX_WG: a launch has min(n_tiles, MAX_WG) workgroups, workgroup g takes the tiles g, g + G, ..


def case_widths(name):
    """(policy widths, value widths) of a case, inputs and outputs included."""
    n_in, ph, vh = CASES[name][:3]
    return (n_in, *ph, 2), (n_in, *vh, 1)


def row_layout(policy_widths, value_widths):
    """(row_floats, tile_rows) as ftgp_train_grad_device lays out an LDS row: every layer's outputs (the input among them) padded to 4
    floats, the longer of the two nets; two delta buffers of ld_max floats, the widest layer output rounded up to 64; four floats more
    where the row would be an even number of float4; 32 rows a tile where they fit 63 KiB, 16 otherwise."""
    act_floats, ld_max = 0, 64
    for widths in (policy_widths, value_widths):
        act_floats = max(act_floats, sum((n + 3) & ~3 for n in widths))
        ld_max = max([ld_max] + [(n + 63) & ~63 for n in widths[1:]])
    row_floats = act_floats + 2 * ld_max
    if (row_floats // 4) % 2 == 0:
        row_floats += 4
    return row_floats, 32 if 32 * row_floats * 4 <= 63 * 1024 else 16


def n_tiles(name):
    B = CASES[name][6]
    R = row_layout(*case_widths(name))[1]
    return (B + R - 1) // R


def ordered_sum(terms, R, G=MAX_WG, wide=False):
    """The sum of one binary32 term per batch row in the order include/ftgp.h gives for the device: a tile's R rows one after the
    other; tile g, g + G, .. into workgroup g of G = min(tiles, 256), in the order it takes them; the workgroups' sums g ascending.
    In binary32, or (wide) carried in binary64 all the way, with a binary64 result.
    (A batch position past the batch adds +0, which changes nothing.)"""
    T = np.float64 if wide else F
    terms = np.asarray(terms, dtype=F)
    tiles = (terms.size + R - 1) // R
    t = np.zeros(tiles * R, dtype=F)
    t[:terms.size] = terms
    t = t.reshape(tiles, R).astype(T)
    tile_sum = np.zeros(tiles, dtype=T)
    for r in range(R):
        tile_sum = (tile_sum + t[:, r]).astype(T)
    G = min(tiles, G)
    group = np.zeros(G, dtype=T)
    for first in range(0, tiles, G):
        turn = tile_sum[first:first + G]
        group[:turn.size] = (group[:turn.size] + turn).astype(T)
    total = T(0.0)
    for g in range(G):
        total = T(total + group[g])
    return total


def ordered_stats(case, R, value32):
    """stats [0], [2] and [4] to the bit: the three whose terms binary32 fixes -- w; w * (0.5 * (e * e)) with e = v - ret on the value
    the forward pass gives to the bit (value32, one per batch row); w where |rho - 1| > clip, which conditions() keeps 1e-4 clear of a
    tie.  S is the binary32 ordered_sum of w; the other two are added up in binary64 along the same order, divided by S in binary64 and
    rounded once.  ([1] and [3] carry the device's exp.)"""
    rows = case["rows"]
    w = (case["weight"][rows] if case["weight"] is not None else np.ones(len(rows))).astype(F)
    e = (np.asarray(value32, dtype=F) - case["ret"][rows]).astype(F)
    t = loss_terms(case, np.float64)
    S = ordered_sum(w, R)
    half_sq = (F(0.5) * (e * e).astype(F)).astype(F)
    over_S = lambda terms: F(ordered_sum(terms, R, wide=True) / np.float64(S))          # noqa: E731
    return S, over_S((w * half_sq).astype(F)), over_S(np.where(np.abs(t["rho"] - 1) > t["c"], w, F(0.0)))


def ratio_span(case):
    """(largest |logp - logq|, whether every rho is finite) over EVERY row of the case's buffers, in the binary32 model: what a test
    that gives rows a weight of 0 needs, since 0 * infinity would be a NaN of its own making."""
    every = dict(case, rows=np.arange(case["n_rows"]), weight=None)
    t = loss_terms(every, np.float32)
    return float(np.abs(t["logp"] - t["logq"]).max()), bool(np.isfinite(t["rho"]).all() and np.isfinite(t["v"]).all())


def turns_tail(name):
    """The rows of the last tile of a turns* case, two tiles past the workgroups."""
    R = row_layout(*case_widths(name))[1]
    return CASES[name][6] - (MAX_WG + 1) * R


def turns_rows(case, R, tail):
    """For the `turns` scenario: (live, dead, weight).  live: 2 * R distinct rows of the buffers, the only ones with a weight (in
    [0.5, 1.5)); dead: every other row, weight 0.  Redrawn until the clip leaves a row free among the first `tail` live rows and in the
    second R of them: every group of live rows a call is made on has a policy gradient that is not zeros."""
    for attempt in range(200):
        rng = np.random.default_rng([7, R, attempt])
        perm = rng.permutation(case["n_rows"]).astype(np.int32)
        live, dead = perm[:2 * R], perm[2 * R:]
        weight = np.zeros(case["n_rows"], dtype=F)
        weight[live] = rng.uniform(0.5, 1.5, 2 * R).astype(F)
        active = loss_terms(dict(case, rows=live, weight=weight))["active"]
        if active[:tail].any() and active[R:].any():
            return live, dead, weight
    raise AssertionError("no draw of live rows left the clip free where it is needed")


def turns_index(dead, B, placed, seed=0):
    """An index of B batch positions: dead rows drawn at random everywhere, but rows[k] at position at + k for every (at, rows) of
    `placed`."""
    index = np.random.default_rng([11, seed, B]).choice(dead, B).astype(np.int32)
    for at, rows in placed:
        assert 0 <= at and at + len(rows) <= B
        index[at:at + len(rows)] = rows
    return index


def make_case(name, seed=0, with_noise=True):
    """A gradient case: nets, buffers of n_rows rows and the batch rows.  `mean` comes from a copy of the policy perturbed by
    0.03 * N(0, 1), so that the clip binds; the seed is redrawn until conditions() holds (not for LOOSE).  with_noise=False: the case
    with noise = None (the draws are made all the same), its seed redrawn until conditions(high_side=False) holds."""
    n_in, ph, vh, hidden, out_act, n_rows, B, how = CASES[name]
    for attempt in range(200):
        rng = np.random.default_rng([seed, attempt, sum(map(ord, name))])
        policy = dict(layers=random_layers(rng, (n_in, *ph, 2)), hidden_act=hidden, out_act=out_act, out_scale=(1.5, 0.6), out_offset=(1.0, 0.0))
        value = dict(layers=random_layers(rng, (n_in, *vh, 1)), hidden_act=hidden, out_act="identity", out_scale=2.0, out_offset=0.25)
        inputs = rng.uniform(-1, 1, (n_rows, n_in)).astype(F)
        old = [((W + 0.03 * rng.standard_normal(W.shape)).astype(F), (b + 0.03 * rng.standard_normal(b.shape)).astype(F)) for W, b in policy["layers"]]
        y = nm.forward(inputs, old, hidden, out_act)
        mean = nm.fmaf(y, np.asarray(policy["out_scale"], dtype=F)[None, :], np.asarray(policy["out_offset"], dtype=F)[None, :])
        noise = rng.standard_normal((n_rows, 2)).astype(F)
        advantage = rng.standard_normal(n_rows).astype(F)
        ret = rng.standard_normal(n_rows).astype(F)
        weight = None
        first_row = 0
        if how == "index":
            rows = rng.integers(0, n_rows, B).astype(np.int32)           # B > n_rows: repeats
            weight = rng.uniform(0.5, 1.5, n_rows).astype(F)
            weight[rng.integers(0, n_rows, n_rows // 8)] = F(0.0)
            index = rows
        else:
            first_row = n_rows - B - 3 if name != "b" else 5
            rows, index = np.arange(first_row, first_row + B, dtype=np.int32), None
        case = dict(name=name, policy=policy, value=value, inputs=inputs, mean=mean, noise=noise if with_noise else None, advantage=advantage,
                    ret=ret, weight=weight, rows=rows, index=index, first_row=first_row, n_rows=n_rows, std=(F(0.3), F(0.1)), clip=F(0.2),
                    value_coef=F(0.5))
        if name in LOOSE or conditions(case, high_side=with_noise) is None:
            return case
    raise AssertionError(f"case {name}: no seed met the batch conditions: {conditions(case, high_side=with_noise)}")


def stat_scales(case):
    """What the error of stats [0] .. [4] is measured against, in binary64.  [0], [2] and [4] are the stats themselves: the issue's form,
    error relative to the reference stat.  [1] and [3] are sum w*|term| / S instead: they are sums of terms of both signs, and the
    rounding error of a sum follows the size of its terms, not of what is left after they cancel -- as the gradient's error is measured
    against the largest element of a tensor, not element by element."""
    t = loss_terms(case, np.float64)
    w, S = t["w"], t["S"]
    clipped = (w * (np.abs(t["rho"] - 1) > t["c"])).sum() / S
    # ([0], [2] and [4] add up terms of one sign: their scale is the stat itself; a clipped fraction of 0 is exact in any order)
    return np.array([S, (w * np.abs(t["s"])).sum() / S, (w * 0.5 * (t["v"] - t["ret"]) ** 2).sum() / S,
                     (w * np.abs(t["logq"] - t["logp"])).sum() / S, clipped if clipped > 0 else 1.0])


def tolerance(case):
    """(g64 policy, g64 value, stats64, rel_ref policy, rel_ref value, rel_ref stats, the stats' scales): the reference and what the same
    model in binary32 loses against it -- per net the largest over its tensors of max|g32 - g64| / max|g64|; for the stats the largest
    over [0] .. [4] of |s32 - s64| / scale (stat_scales)."""
    gp, gv, st = loss_and_grad(case, np.float64)
    gp32, gv32, st32 = loss_and_grad(case, np.float32)
    rel = lambda g64, g32: max(np.abs(a32.astype(np.float64) - a64).max() / np.abs(a64).max() for p64, p32 in zip(g64, g32) for a64, a32 in zip(p64, p32))   # noqa: E731
    scales = stat_scales(case)
    rs = (np.abs(st32[:5].astype(np.float64) - st[:5]) / scales).max()
    return gp, gv, st, rel(gp, gp32), rel(gv, gv32), float(rs), scales
