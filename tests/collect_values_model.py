"""Collected rollouts with values (include/ftgp.h: ftgp_set_value_net, ftgp_collect_values_device, ftgp_gae_device), restated in numpy
from the header's text -- not from csrc/ftgp_net.h and not from the kernels.  Binary32 with one rounding per written operation; fmaf is
the exact one of tests/net_model.py; the layers are that model's restatement of "Layers".
"""
import numpy as np

from tests import net_model as nm

F = np.float32


def value(vnet, x):
    """v float32 [...]: the value net `vnet` = dict(layers, hidden_act, out_act, out_scale, out_offset) on inputs x [..., n_in]:
    y = the single output of the last layer, v = fmaf(y, out_scale, out_offset); no guard."""
    x = np.asarray(x, dtype=F)
    flat = x.reshape(-1, x.shape[-1])
    with np.errstate(all="ignore"):
        y = nm.forward(flat, vnet["layers"], vnet.get("hidden_act", "tanh"), vnet.get("out_act", "identity"))
        assert y.shape[1] == 1
        v = nm.fmaf(y[:, 0], F(vnet.get("out_scale", 1.0)), F(vnet.get("out_offset", 0.0)))
    return v.reshape(x.shape[:-1]).astype(F)


def gae(reward, val, next_val, terminated, truncated, gamma, lam):
    """(advantage, ret) float32 [T, n_envs, n_ext] of the advantage scan.  gl = gamma * lam rounded once; for t = T-1 down to 0:
    nv = term ? 0 : next_value[t]; d = fmaf(gamma, nv, reward[t]) - value[t]; A = (t == T-1 or term or trunc) ? d : fmaf(gl, A_next, d);
    advantage[t] = A; ret[t] = A + value[t]."""
    reward, val, next_val = (np.asarray(a, dtype=F) for a in (reward, val, next_val))
    term = np.asarray(terminated).astype(bool)[:, :, None]
    trunc = np.asarray(truncated).astype(bool)[:, :, None]
    T = reward.shape[0]
    g = F(gamma)
    gl = F(F(gamma) * F(lam))
    adv, ret = np.zeros_like(reward), np.zeros_like(reward)
    A = np.zeros_like(reward[0])
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            nv = np.where(term[t], F(0.0), next_val[t]).astype(F)
            d = (nm.fmaf(g, nv, reward[t]) - val[t]).astype(F)
            A = d if t == T - 1 else np.where(term[t] | trunc[t], d, nm.fmaf(gl, A, d)).astype(F)
            adv[t] = A
            ret[t] = (A + val[t]).astype(F)
    return adv, ret


def random_value_net(rng, widths, hidden_act="tanh", out_act="identity", out_scale=1.0, out_offset=0.0, gain=1.0):
    """A random value net of the given widths (n_in, ..., 1): weights ~ N(0, gain / sqrt(n_in)), biases ~ N(0, 0.1)."""
    assert widths[-1] == 1
    layers = []
    for n_in, n_out in zip(widths[:-1], widths[1:]):
        layers.append(((rng.standard_normal((n_out, n_in)) * gain / np.sqrt(n_in)).astype(F), (0.1 * rng.standard_normal(n_out)).astype(F)))
    return dict(layers=layers, hidden_act=hidden_act, out_act=out_act, out_scale=out_scale, out_offset=out_offset)


def value_fields(vnet):
    return {k: v for k, v in vnet.items() if k != "layers"}


def scan_cases(seed=17):
    """name -> dict(reward, value, next_value [T, n_envs, n_ext], terminated, truncated uint8 [T, n_envs], gamma, lam): the crafted rows
    of the scan -- random rows with a NaN and both infinities in reward and value and random masks; T = 1; every step terminated;
    truncated steps only; gamma and lam at 0 and 1."""
    rng = np.random.default_rng(seed)

    def rows(T, n_envs, n_ext, p_term=0.15, p_trunc=0.15, special=True):
        r, v, nv = (rng.standard_normal((T, n_envs, n_ext)).astype(F) for _ in range(3))
        if special:
            vals = np.array([np.nan, np.inf, -np.inf], dtype=F)
            for a in (r, v):
                a.reshape(-1)[rng.choice(a.size, len(vals), replace=False)] = vals           # three places, all different
        term = (rng.random((T, n_envs)) < p_term).astype(np.uint8)
        trunc = (rng.random((T, n_envs)) < p_trunc).astype(np.uint8)
        return dict(reward=r, value=v, next_value=nv, terminated=term, truncated=trunc)

    cases = {
        "random": dict(rows(16, 7, 1), gamma=0.99, lam=0.95),
        "random_two_waves_and_a_tail": dict(rows(9, 65, 2), gamma=0.97, lam=0.9),           # 130 rows
        "one_decision": dict(rows(1, 7, 1), gamma=0.99, lam=0.95),
        "all_terminated": dict(rows(6, 7, 1, p_term=2.0, p_trunc=0.0), gamma=0.99, lam=0.95),
        "truncated_only": dict(rows(8, 7, 1, p_term=0.0, p_trunc=0.4), gamma=0.99, lam=0.95),
    }
    for g in (0.0, 1.0):
        for l in (0.0, 1.0):
            cases[f"gamma_{g:g}_lam_{l:g}"] = dict(rows(8, 7, 1), gamma=g, lam=l)
    return cases


def hand_row():
    """One row in exactly representable numbers: gamma = lam = 1/2, rewards and values small powers of two, a termination at t = 2 and a
    truncation at t = 4 inside T = 6.  Returns the case and the advantages of the textbook recursion computed in binary64:
    delta_t = r_t + gamma * (1 - term_t) * V(s_t+1) - V(s_t), A_t = delta_t + gamma * lam * (1 - end_t) * A_t+1 -- every intermediate
    is a multiple of 2^-12 below 2^4, exact in binary32 and in binary64 alike."""
    T = 6
    reward = np.array([1.0, 0.5, 2.0, 0.25, 1.0, 4.0], dtype=F).reshape(T, 1, 1)
    val = np.array([0.5, 2.0, 1.0, 0.125, 4.0, 0.25], dtype=F).reshape(T, 1, 1)
    next_val = np.array([2.0, 1.0, 8.0, 4.0, 0.5, 1.0], dtype=F).reshape(T, 1, 1)      # (next_value[2] must not count: terminated)
    term = np.array([0, 0, 1, 0, 0, 0], dtype=np.uint8).reshape(T, 1)
    trunc = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint8).reshape(T, 1)
    gamma = lam = 0.5
    A = np.zeros(T + 1, dtype=np.float64)
    for t in range(T - 1, -1, -1):
        r, v, nv = float(reward[t, 0, 0]), float(val[t, 0, 0]), float(next_val[t, 0, 0])
        delta = r + gamma * (1 - int(term[t, 0])) * nv - v
        cont = 0 if (t == T - 1 or term[t, 0] or trunc[t, 0]) else 1
        A[t] = delta + gamma * lam * cont * A[t + 1]
    case = dict(reward=reward, value=val, next_value=next_val, terminated=term, truncated=trunc, gamma=gamma, lam=lam)
    return case, A[:T].reshape(T, 1, 1), (A[:T] + val[:, 0, 0].astype(np.float64)).reshape(T, 1, 1)
