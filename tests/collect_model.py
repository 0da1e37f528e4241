"""Step 1 ("Act") of a collected decision, restated in numpy from the text of include/ftgp.h ("Collected rollouts") -- not from
csrc/ftgp_net.h.  The inputs and the layers are the network driver's (tests/net_model.py, imported); new here are the mean, the noise,
the clip and the guard.  Everything is binary32 with one rounding per written operation; fmaf is exact (net_model.fmaf).
"""
import numpy as np

from tests import net_model as nm

F = np.float32


def same_bits(a, b):
    """Equal to the bit, element-wise; a NaN equals a NaN (the header does not fix a NaN's payload)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    if not same_bits(got, want):
        bad = np.argwhere(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, first at {i}: got {got[i]!r} ({got[i].view(np.uint32):#x}), "
                             f"want {want[i]!r} ({want[i].view(np.uint32):#x})")


def inputs(net, scans, pose, ctrl):
    """x float32 [n_cars, n_in]: "Scan input" and "State input" of ftgp_set_net on ftgp_get_lidar / ftgp_get_pose / ftgp_get_ctrl rows."""
    x = nm.beams(scans, net["pool"], net["max_range"], net["beam_first"], net["n_beams"])
    if net.get("use_state"):
        x = np.concatenate([x, nm.state_inputs(pose, ctrl)], axis=1)
    return x.astype(F)


def mean(y, out_scale, out_offset):
    """m_k = fmaf(y_k, out_scale[k], out_offset[k]); not guarded."""
    return nm.fmaf(np.asarray(y, dtype=F)[:, :2], np.asarray(out_scale, dtype=F)[None, :], np.asarray(out_offset, dtype=F)[None, :])


def action(m, std, noise, lo, hi):
    """a_k = fmaf(std[k], noise_k, m_k); a_k = a_k < lo[k] ? lo[k] : (a_k > hi[k] ? hi[k] : a_k); if a_0 or a_1 is not finite, both
    are 0.  noise None = zeros."""
    m = np.asarray(m, dtype=F)
    std, lo, hi = (np.asarray(v, dtype=F)[None, :] for v in (std, lo, hi))
    z = np.zeros_like(m) if noise is None else np.asarray(noise, dtype=F)
    with np.errstate(all="ignore"):
        a = nm.fmaf(np.broadcast_to(std, m.shape), z, m)
        a = np.where(a < lo, lo, np.where(a > hi, hi, a)).astype(F)
    ok = np.isfinite(a).all(axis=1)
    return np.where(ok[:, None], a, F(0.0)).astype(F)


def act(net, scans, pose, ctrl, finished, std, noise, lo, hi):
    """(x, mean, action) of every car: a finished car gets mean = action = (0, 0), and its inputs all the same."""
    x = inputs(net, scans, pose, ctrl)
    y = nm.forward(x, net["layers"], net.get("hidden_act", "tanh"), net.get("out_act", "tanh"))
    m = mean(y, net.get("out_scale", (1, 1)), net.get("out_offset", (0, 0)))
    a = action(m, std, noise, lo, hi)
    fin = np.asarray(finished, dtype=bool)[:, None]
    return x, np.where(fin, F(0.0), m).astype(F), np.where(fin, F(0.0), a).astype(F)


def element_cases(seed=5, n=400):
    """(y, noise, scale, offset, std, lo, hi) sets for the host harness: ordinary draws, NaN and +-inf noise, NaN and +-inf outputs,
    lo == hi, std = 0."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n, 2)).astype(F)
    z = rng.standard_normal((n, 2)).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e38, -1e38], dtype=F)
    z[rng.integers(0, n, 60), rng.integers(0, 2, 60)] = special[rng.integers(0, 3, 60)]
    y[rng.integers(0, n, 40), rng.integers(0, 2, 40)] = special[rng.integers(0, 7, 40)]
    base = dict(scale=(3.5, 0.6), offset=(3.5, 0.0))
    return {
        "plain": dict(y=y, noise=z, std=(0.5, 0.2), lo=(0.0, -0.5), hi=(6.0, 0.5), **base),
        "wide": dict(y=y, noise=z, std=(1.5, 1.0), lo=(-1e30, -1e30), hi=(1e30, 1e30), **base),
        "lo_is_hi": dict(y=y, noise=z, std=(0.5, 0.2), lo=(1.25, -0.0), hi=(1.25, 0.0), **base),
        "std_zero": dict(y=y, noise=z, std=(0.0, 0.0), lo=(0.0, -0.5), hi=(6.0, 0.5), **base),
        "one_std_zero": dict(y=y, noise=z, std=(0.0, 0.3), lo=(0.5, -0.25), hi=(2.0, 0.25), scale=(1.0, 1.0), offset=(0.0, 0.0)),
    }
