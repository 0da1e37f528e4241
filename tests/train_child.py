"""Child process of tests/test_train.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/train_child.py <scenario> [json options]

The criteria (include/ftgp.h "Training on the device"): new_mean and new_value equal tests/net_model.py to the bit; the gradient and the
stats lie within four times the distance of the binary32 model from the binary64 one (tests/train_model.py: tolerance); Adam equals the
model's element step to the bit on the gradients read back; a batch whose rows have weight 0 but for one or two tiles gives exactly the
gradient and the stats of those tiles' rows alone, whichever workgroup's whichever turn they fall on (turns).
"""
import functools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: one HIP runtime per process)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from ft_grandprix_amd.track import load_track  # noqa: E402
from tests import collect_model as cmod  # noqa: E402
from tests import net_model as nm  # noqa: E402
from tests import train_model as tm  # noqa: E402

ERR_ARG, ERR_STATE = -1, -4
DEV = "cuda"
F = np.float32
# the slot description that gives a net n_in inputs: (n_rays, pool, max_range, beam_first, n_beams, use_state)
INPUTS = {85: (1080, 10, 10.0, 14, 80, True), 1: (64, 4, 3.0, 2, 1, False), 256: (1344, 4, 8.0, 42, 251, True), 33: (1080, 10, 10.0, 14, 28, True),
          17: (64, 4, 3.0, 2, 12, True), 104: (1344, 4, 8.0, 42, 99, True), 108: (1344, 4, 8.0, 42, 103, True)}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return 0 if t is None else t.data_ptr()


def make_env(case, n_envs=8, begin=True):
    """A handle whose slot 0 is the case's policy with its value net, and (begin) a trainer."""
    n_in = case["inputs"].shape[1]
    n_rays, pool, M, first, n_beams, use_state = INPUTS[n_in]
    env = capi.Env(capi.load(), load_track("small-circle"), n_envs=n_envs, n_rays=n_rays, spawn_mode=1, seed=5)
    p, v = case["policy"], case["value"]
    env.set_net(0, p["layers"], pool=pool, max_range=M, beam_first=first, n_beams=n_beams, use_state=use_state, hidden_act=p["hidden_act"],
                out_act=p["out_act"], out_scale=p["out_scale"], out_offset=p["out_offset"])
    env.set_value_net(0, v["layers"], hidden_act=v["hidden_act"], out_act=v["out_act"], out_scale=v["out_scale"], out_offset=v["out_offset"])
    if begin:
        env.train_begin(0)
    return env


class Batch:
    """The device buffers of a case and one ftgp_train_grad_device call on them."""

    def __init__(self, case):
        self.case = case
        self.t = {k: dev(case[k]) for k in ("inputs", "mean", "noise", "advantage", "ret", "weight", "index")}
        B = len(case["rows"])
        self.B = B
        self.stats, self.new_mean, self.new_value = (torch.full(s, -7.0, device=DEV) for s in ((capi.TRAIN_STATS,), (B, 2), (B,)))

    def args(self, stream=0, **over):
        c, t = self.case, self.t
        kw = dict(slot=0, first_row=int(c["first_row"]), index=ptr(t["index"]), inputs=ptr(t["inputs"]), mean=ptr(t["mean"]), noise=ptr(t["noise"]),
                  advantage=ptr(t["advantage"]), ret=ptr(t["ret"]), weight=ptr(t["weight"]), std=c["std"], clip=c["clip"], value_coef=c["value_coef"],
                  stats=ptr(self.stats), new_mean=ptr(self.new_mean), new_value=ptr(self.new_value), stream=stream)
        kw.update(over)
        return capi.train_batch(int(c["n_rows"]), self.B, **kw)

    def grad(self, env, stream=0, **over):
        env.train_grad_device(self.args(stream, **over))
        torch.cuda.synchronize()
        return self.stats.cpu().numpy().copy()


def widths_of(net):
    return (net["layers"][0][0].shape[1],) + tuple(W.shape[0] for W, _ in net["layers"])


def grads_of(env, case, what=capi.TRAIN_GRAD):
    pol, val, t = env.train_get(0, what)
    return tm.unflat(pol, widths_of(case["policy"])), tm.unflat(val, widths_of(case["value"])), t


def forward_bits(what, case, b):
    """new_mean and new_value against tests/net_model.py on the batch rows."""
    p, v, x = case["policy"], case["value"], case["inputs"][case["rows"]]
    y = nm.forward(x, p["layers"], p["hidden_act"], p["out_act"])
    want = nm.fmaf(y, np.asarray(p["out_scale"], dtype=F)[None, :], np.asarray(p["out_offset"], dtype=F)[None, :])
    cmod.assert_same_bits(b.new_mean.cpu().numpy(), want, f"{what}: new_mean against the model")
    yv = nm.forward(x, v["layers"], v["hidden_act"], v["out_act"])
    want_value = nm.fmaf(yv[:, 0], F(v["out_scale"]), F(v["out_offset"]))
    cmod.assert_same_bits(b.new_value.cpu().numpy(), want_value, f"{what}: new_value against the model")
    return want, want_value


def padding_is_zero(what, env, which, caller):
    """The raw library layout of both nets (capi.Env.train_get_raw): the columns behind n_out are zeros (+0 bits), the others are what
    the caller's layout `caller` = (policy layers, value layers) holds, transposed."""
    seen = 0
    for net, raw, lay in zip(("policy", "value"), env.train_get_raw(0, which), caller):
        for l, ((Wt, b), (W, bias)) in enumerate(zip(raw, lay)):
            n_out, n_in = W.shape
            assert Wt.shape[0] == n_in and Wt.shape[1] % 64 == 0 and Wt.shape[1] >= n_out
            cmod.assert_same_bits(np.ascontiguousarray(Wt[:, :n_out].T), np.asarray(W, dtype=F), f"{what}: {net} layer {l} W through the raw read")
            cmod.assert_same_bits(b[:n_out], np.asarray(bias, dtype=F), f"{what}: {net} layer {l} b through the raw read")
            pad = np.concatenate([Wt[:, n_out:].ravel(), b[n_out:]])
            assert pad.size == (n_in + 1) * (Wt.shape[1] - n_out) and not pad.view(np.uint32).any(), f"{what}: {net} layer {l}: padding is not zeros"
            seen += pad.size
    assert seen > 0
    return seen


def gradient(opt):
    """Every case of tm.CASES: the gradient and the stats within 4 * rel_ref of the binary64 model, the forward pass to the bit.
    noise = false: the case with noise = None in the model and NULL in the call."""
    name = opt["only"]
    with_noise = opt.get("noise", True)
    case = tm.make_case(name, with_noise=with_noise)
    if not with_noise:
        assert case["noise"] is None and tm.conditions(case, high_side=False) is None
        name += " without noise"
    gp, gv, st, rel_p, rel_v, rel_s, scales = tm.tolerance(case)
    env = make_env(case)
    b = Batch(case)
    stats = b.grad(env)
    _, value32 = forward_bits(name, case, b)
    # S, the value loss and the clipped fraction: binary32 sums in the order the header gives, to the bit
    R = tm.row_layout(widths_of(case["policy"]), widths_of(case["value"]))[1]
    ordered = tm.ordered_stats(case, R, value32)
    print(f"case {name}: stats [0], [2], [4] = {[float(stats[q]) for q in (0, 2, 4)]} against the sums in the device's order {[float(x) for x in ordered]}")
    cmod.assert_same_bits(stats[[0, 2, 4]], np.array(ordered, dtype=F), f"{name}: stats [0], [2] and [4] against the binary32 sums in the device's order")
    dp, dv, t = grads_of(env, case)
    assert t == 0
    worst = {}
    for net, g64, gdev, rel in (("policy", gp, dp, rel_p), ("value", gv, dv, rel_v)):
        assert rel > 0, f"{name}: the binary32 model of the {net} gradient equals the binary64 one: no tolerance follows"
        for l, (ref, got) in enumerate(zip(g64, gdev)):
            for part, r64, g in zip("Wb", ref, got):
                err = np.abs(g.astype(np.float64) - r64).max() / np.abs(r64).max()
                worst[net] = max(worst.get(net, 0.0), err / rel)
                print(f"case {name}: {net} layer {l} {part}: max|g_dev - g64| / max|g64| = {err:.3e}, rel_ref = {rel:.3e}, ratio {err / rel:.2f}")
    serr = np.abs(stats[:5].astype(np.float64) - st[:5]) / scales           # against the size of what a stat adds up (tm.stat_scales)
    print(f"case {name}: stats {stats.tolist()} against {st.tolist()}: errors / scale {serr.tolist()}, rel_ref = {rel_s:.3e}")
    assert rel_s > 0, f"{name}: the binary32 model of the stats equals the binary64 one: no tolerance follows"
    print(f"case {name}: ratios policy {worst['policy']:.2f} value {worst['value']:.2f} stats {serr.max() / rel_s:.2f}")
    assert worst["policy"] <= 4.0 and worst["value"] <= 4.0, f"{name}: a gradient lies further than 4 * rel_ref from the binary64 model: {worst}"
    assert (serr <= 4.0 * rel_s).all(), f"{name}: a stat lies further than 4 * rel_ref = {4 * rel_s:.3e} from the binary64 model: {serr}"
    assert stats[5] == 0 and stats[6] == 0 and stats[7] == 0
    # the library layout's padding, read as raw device memory: zeros in the gradient, and zeros in the parameters after an Adam step
    padding_is_zero(f"{name}: the gradient", env, capi.TRAIN_RAW_GRAD, (dp, dv))
    env.train_adam_device(0, 1e-3)
    _, pl = env.net(0)
    _, vl = env.get_value_net(0)
    padding_is_zero(f"{name}: the parameters after Adam", env, capi.TRAIN_RAW_PARAMS, (pl, vl))
    assert not np.array_equal(tm.flat(pl), tm.flat(case["policy"]["layers"])), "Adam moved the parameters"
    env.close()
    print(f"gradient {name} ok")


def turns(opt):
    """What a tile adds to the gradient does not depend on whose turn it is: the nets of turns32 (tiles of 32 rows) or turns16 (of 16),
    one handle, every comparison exact.  Only the rows tm.turns_rows calls live have a weight; every other batch position names a
    real row whose weight is 0.  Such a row's deltas are +-0, and adding +-0 to a partial sum, in a workgroup or across workgroups, is
    exact: a batch of hundreds of tiles must give the values of a batch of its live rows alone."""
    name = opt["only"]
    case = tm.make_case(name)
    R = tm.row_layout(*tm.case_widths(name))[1]
    G = tm.MAX_WG
    B = tm.CASES[name][6]
    tail = tm.turns_tail(name)                                         # the live rows of the ragged last tile
    assert opt["rows"] == R and tm.n_tiles(name) == G + 2 and 0 < tail < R and B == (G + 1) * R + tail
    span, finite = tm.ratio_span(case)
    assert finite and span < 80.0, f"{name}: a row of weight 0 would make a NaN of the test's own: {span}, {finite}"
    live, dead, weight = tm.turns_rows(case, R, tail)
    a, pair = live[:R], live
    env = make_env(case)
    # the forward pass of every row of the buffers, once
    p, v = case["policy"], case["value"]
    y = nm.forward(case["inputs"], p["layers"], p["hidden_act"], p["out_act"])
    mean_of = nm.fmaf(y, np.asarray(p["out_scale"], dtype=F)[None, :], np.asarray(p["out_offset"], dtype=F)[None, :])
    yv = nm.forward(case["inputs"], v["layers"], v["hidden_act"], v["out_act"])
    value_of = nm.fmaf(yv[:, 0], F(v["out_scale"]), F(v["out_offset"]))

    def run(what, index, null=False):
        """(stats, policy gradient, value gradient) of one call on `index`; new_mean and new_value against the model to the bit."""
        index = np.asarray(index, dtype=np.int32)
        b = Batch(dict(case, index=index, rows=index, weight=weight, first_row=0))
        stats = b.grad(env, **(dict(stats=0, new_mean=0, new_value=0) if null else {}))
        g = env.train_get(0)
        if null:
            assert (stats == -7.0).all() and (b.new_mean.cpu().numpy() == -7.0).all() and (b.new_value.cpu().numpy() == -7.0).all()
            return None, g[0], g[1]
        ok = (index >= 0) & (index < case["n_rows"])
        rows = np.where(ok, index, 0)
        cmod.assert_same_bits(b.new_mean.cpu().numpy(), np.where(ok[:, None], mean_of[rows], F(0.0)), f"{name} {what}: new_mean against the model")
        cmod.assert_same_bits(b.new_value.cpu().numpy(), np.where(ok, value_of[rows], F(0.0)), f"{name} {what}: new_value against the model")
        assert stats[5] == 0 and stats[6] == np.count_nonzero(~ok) and stats[7] == 0, (what, stats)
        return stats, g[0], g[1]

    def same(what, got, want):
        if got[0] is not None:
            assert np.array_equal(got[0][:5], want[0][:5]), f"{name} {what}: stats {got[0]} against {want[0]}"
        for net, g, w in (("policy", got[1], want[1]), ("value", got[2], want[2])):
            assert np.array_equal(g, w), f"{name} {what}: the {net} gradient differs in {np.count_nonzero(g != w)} of {g.size} elements, by up to {np.abs(g - w).max():.3e}"
        print(f"{name} {what}: equal")

    def batch(n_batch, placed, seed=0):
        return tm.turns_index(dead, n_batch, placed, seed)

    ref = run("the live tile alone", a)
    ref_tail = run("the ragged tile's live rows alone", a[:tail])
    ref_pair = run("two live tiles alone", pair)
    for r in (ref, ref_tail, ref_pair):
        assert r[0][0] > 0 and np.abs(r[1]).max() > 0 and np.abs(r[2]).max() > 0 and np.isfinite(r[1]).all() and np.isfinite(r[2]).all()
    # (stats[0] = S: a tile's weights added one after the other in binary32, then the tiles)
    one_by_one = lambda w: functools.reduce(lambda s, x: F(s + x), w, F(0.0))          # noqa: E731
    assert ref[0][0] == one_by_one(weight[a]) and ref_tail[0][0] == one_by_one(weight[a[:tail]])
    assert ref_pair[0][0] == F(one_by_one(weight[a]) + one_by_one(weight[live[R:]]))
    assert not np.array_equal(ref[1], ref_tail[1]) and not np.array_equal(ref[1], ref_pair[1]) and not np.array_equal(ref[2], ref_pair[2])
    # 1. 258 tiles, the only live rows in tile t: the first turn of workgroup 0 and of the last workgroup, the second turn of workgroup 0,
    #    the ragged last tile
    for t in (0, G - 1, G, G + 1):
        rows = a if t <= G else a[:tail]
        same(f"live tile {t} of {G + 2}", run(f"tile {t}", batch(B, [(t * R, rows)], t)), ref if t <= G else ref_tail)
    # 2. a third turn, behind a second turn of zeros
    same(f"live tile {2 * G} of {3 * G + 1}", run(f"tile {2 * G}", batch((3 * G + 1) * R, [(2 * G * R, a)])), ref)
    # 3. two live tiles of one workgroup: a, then += b, against a + b of the reduce over two workgroups -- the same one rounding
    same(f"live tiles 3 and {G + 3} of {G + 4}", run("tiles 3 and 259", batch((G + 4) * R, [(3 * R, a), ((G + 3) * R, live[R:])])), ref_pair)
    # 4. row numbers -1 and n_rows inside the live tile of a second turn: counted, and the batch that has dead rows in their place
    holed = a.copy(); holed[[R // 4, R - 3]] = dead[:2]
    refused = holed.copy(); refused[[R // 4, R - 3]] = (-1, case["n_rows"])
    with_dead = run("dead rows at two positions", batch(B, [(G * R, holed)], 4))
    with_refused = run("row numbers -1 and n_rows", batch(B, [(G * R, refused)], 4))
    assert with_refused[0][6] == 2 and with_dead[0][6] == 0
    same(f"row numbers -1 and n_rows in tile {G}", with_refused, with_dead)
    assert not np.array_equal(with_dead[2], ref[2])
    # 5. stats, new_mean and new_value NULL (behind a call with another gradient): the same gradient
    same(f"live tile {G} with stats, new_mean and new_value NULL", run("NULL outputs", batch(B, [(G * R, a)], G), null=True), ref)
    env.close()
    print(f"turns {name} ok")


def collected(opt):
    """A real ftgp_collect_values_device rollout, then the gradient call on all its rows with unchanged parameters."""
    from tests import collect_child as cc
    case = tm.make_case("d")
    n_envs, T = 16, 4
    env = make_env(case, n_envs=n_envs, begin=False)
    env.device_io_config(["agent"], max_episode_steps=1000, action_repeat=1, auto_reset=True)
    n_in, lead = 33, (T, n_envs, 1)
    z = cc.zeros
    inputs, mean, action, reward = z(lead + (n_in,)), z(lead + (2,)), z(lead + (2,)), z(lead)
    term, trunc = z((T, n_envs), torch.uint8), z((T, n_envs), torch.uint8)
    value, next_value, adv, ret = z(lead), z(lead), z(lead), z(lead)
    noise = dev(np.random.default_rng(3).standard_normal(lead + (2,)).astype(F))
    std = (0.3, 0.1)
    env.collect_values_device(T, inputs.data_ptr(), mean.data_ptr(), action.data_ptr(), reward.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                              value.data_ptr(), next_value.data_ptr(), advantage=adv.data_ptr(), ret=ret.data_ptr(), std=std, noise=noise.data_ptr())
    torch.cuda.synchronize()
    assert not env.progress()[:, 4].any(), "no car finished inside the rollout"
    env.train_begin(0)
    n = T * n_envs
    stats, new_mean, new_value = z((8,)), z((n, 2)), z((n,))
    env.train_grad_device(capi.train_batch(n, n, inputs=inputs.data_ptr(), mean=mean.data_ptr(), noise=noise.data_ptr(), advantage=adv.data_ptr(),
                                           ret=ret.data_ptr(), std=std, clip=0.2, value_coef=0.5, stats=stats.data_ptr(),
                                           new_mean=new_mean.data_ptr(), new_value=new_value.data_ptr()))
    torch.cuda.synchronize()
    cmod.assert_same_bits(new_mean.cpu().numpy(), mean.cpu().numpy().reshape(n, 2), "new_mean against the rollout's mean")
    cmod.assert_same_bits(new_value.cpu().numpy(), value.cpu().numpy().reshape(n), "new_value against the rollout's value")
    s = stats.cpu().numpy()
    assert np.abs(noise.cpu().numpy()).min() > 0 and np.unique(mean.cpu().numpy()).size > n
    assert s[0] == n and s[3] == 0.0 and s[4] == 0.0 and s[5] == 0.0 and s[6] == 0.0, s
    env.close()
    print("collected ok")


def adam(opt):
    """Three grad + Adam steps: the parameters, the moments and t against the model's Adam on the gradients read back; then the step
    kernel and ftgp_policy_eval run what Adam wrote."""
    case = tm.make_case("d")
    env = make_env(case, n_envs=8)
    b = Batch(case)
    pw, vw = widths_of(case["policy"]), widths_of(case["value"])
    p = [tm.flat(case["policy"]["layers"]), tm.flat(case["value"]["layers"])]
    m = [np.zeros_like(x) for x in p]
    v = [np.zeros_like(x) for x in p]
    lr = 0.01
    for step in range(1, 4):
        b.grad(env)
        g = env.train_get(0, capi.TRAIN_GRAD)
        assert g[2] == step - 1
        env.train_adam_device(0, lr)
        sc = tm.adam_scalars(0.9, 0.999, lr, step)
        for k in range(2):
            p[k], m[k], v[k] = tm.adam_step(p[k], m[k], v[k], g[k], sc, 1e-8)
        gm, gv = env.train_get(0, capi.TRAIN_M), env.train_get(0, capi.TRAIN_V)
        assert gm[2] == step and gv[2] == step
        _, pl = env.net(0)
        _, vl = env.get_value_net(0)
        for k, got_p in enumerate((tm.flat(pl), tm.flat(vl))):
            cmod.assert_same_bits(got_p, p[k], f"step {step}: parameters of net {k}")
            cmod.assert_same_bits(gm[k], m[k], f"step {step}: m of net {k}")
            cmod.assert_same_bits(gv[k], v[k], f"step {step}: v of net {k}")
        assert np.abs(g[0]).max() > 0 and np.abs(g[1]).max() > 0
    assert not np.array_equal(p[0], tm.flat(case["policy"]["layers"]))
    # the next launch that names the slot runs the new network
    rng = np.random.default_rng(9)
    scans = nm.eval_scans(rng, env.n_cars, env.n_rays, 10.0)
    n_rays, pool, M, first, n_beams, use_state = INPUTS[33]
    net = dict(layers=tm.unflat(p[0], pw), pool=pool, max_range=M, beam_first=first, n_beams=n_beams, use_state=use_state,
               hidden_act=case["policy"]["hidden_act"], out_act=case["policy"]["out_act"], out_scale=case["policy"]["out_scale"],
               out_offset=case["policy"]["out_offset"])
    want = nm.evaluate(net, scans, env.pose(), env.ctrl())
    np.testing.assert_array_equal(env.policy_eval("net0", scans), want, err_msg="ftgp_policy_eval after three Adam steps")
    # (the case has a new trainer's value net behind it as well)
    b.grad(env)
    x = case["inputs"][case["rows"]]
    yv = nm.forward(x, tm.unflat(p[1], vw), case["value"]["hidden_act"], case["value"]["out_act"])
    cmod.assert_same_bits(b.new_value.cpu().numpy(), nm.fmaf(yv[:, 0], F(case["value"]["out_scale"]), F(case["value"]["out_offset"])), "new_value after three steps")
    env.close()
    print("adam ok")


def determinism(opt):
    case = tm.make_case("a")
    env = make_env(case)
    b = Batch(case)
    s0 = b.grad(env)
    g0 = env.train_get(0)
    s1 = b.grad(env)
    g1 = env.train_get(0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.randn((2048, 2048), device=DEV)
        for _ in range(10):
            big = torch.tanh(big @ big)
        s2 = b.grad(env, stream=side.cuda_stream)
    g2 = env.train_get(0)
    for s, g, what in ((s1, g1, "the same call again"), (s2, g2, "on another stream behind unrelated work")):
        assert s.tobytes() == s0.tobytes(), f"{what}: stats {s} against {s0}"
        assert g[0].tobytes() == g0[0].tobytes() and g[1].tobytes() == g0[1].tobytes(), f"{what}: the gradient's bytes differ"
    assert np.abs(g0[0]).max() > 0
    env.close()
    print("determinism ok")


def guards(opt):
    case = tm.make_case("d")
    env = make_env(case)
    # a NaN advantage in one batch row: the flag, and Adam leaves everything as it was
    bad = dict(case)
    bad["advantage"] = case["advantage"].copy(); bad["advantage"][case["rows"][7]] = np.nan
    b = Batch(case)
    b.grad(env); env.train_adam_device(0, 0.01)                       # (one good step: the moments are not zeros)
    before = [env.train_get(0, w)[:2] for w in (capi.TRAIN_M, capi.TRAIN_V)] + [(tm.flat(env.net(0)[1]), tm.flat(env.get_value_net(0)[1]))]
    s = Batch(bad).grad(env)
    assert s[5] == 1.0, s
    env.train_adam_device(0, 0.01)
    after = [env.train_get(0, w)[:2] for w in (capi.TRAIN_M, capi.TRAIN_V)] + [(tm.flat(env.net(0)[1]), tm.flat(env.get_value_net(0)[1]))]
    for x, y in zip(before, after):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes(), "Adam moved something under a non-finite gradient"
    assert env.train_get(0)[2] == 2, "t still advances"
    # row numbers -1 and n_rows at the end of an index: counted, never read, and the gradient of the batch without them
    rows = case["rows"].astype(np.int32)
    good = dict(case); good["index"] = rows
    s_good = Batch(good).grad(env)
    g_good = env.train_get(0)
    refused = dict(case); refused["index"] = np.concatenate([rows, np.array([-1, case["n_rows"]], dtype=np.int32)]); refused["rows"] = refused["index"]
    br = Batch(refused)
    s_ref = br.grad(env)
    g_ref = env.train_get(0)
    assert s_ref[6] == 2.0 and s_good[6] == 0.0 and s_ref[5] == 0.0, (s_ref, s_good)
    np.testing.assert_array_equal(s_ref[:5], s_good[:5])
    np.testing.assert_array_equal(g_ref[0], g_good[0]); np.testing.assert_array_equal(g_ref[1], g_good[1])
    assert (br.new_mean.cpu().numpy()[-2:] == 0).all() and (br.new_value.cpu().numpy()[-2:] == 0).all()
    # all weights 0: zeros
    zero = dict(case); zero["weight"] = np.zeros(case["n_rows"], dtype=F)
    s_zero = Batch(zero).grad(env)
    g_zero = env.train_get(0)
    assert not s_zero.any() and not g_zero[0].any() and not g_zero[1].any(), s_zero
    env.close()
    print("guards ok")


def optimises(opt):
    case = dict(tm.make_case("d"))
    case["advantage"] = np.zeros_like(case["advantage"])
    env = make_env(case)
    b = Batch(case)
    first = last = None
    for step in range(60):
        s = b.grad(env)
        first = s[2] if first is None else first
        last = s[2]
        env.train_adam_device(0, 1e-2)
    print(f"value loss {first} -> {last}")
    assert last <= 0.5 * first, (first, last)
    env.close()
    # value_coef = 0, positive advantages, mean from the policy in force (unclipped rows): the surrogate loss falls
    case = dict(tm.make_case("d"))
    p = case["policy"]
    y = nm.forward(case["inputs"], p["layers"], p["hidden_act"], p["out_act"])
    case["mean"] = nm.fmaf(y, np.asarray(p["out_scale"], dtype=F)[None, :], np.asarray(p["out_offset"], dtype=F)[None, :])
    case["advantage"] = np.abs(case["advantage"]) + F(0.1)
    case["value_coef"] = F(0.0)
    env = make_env(case)
    b = Batch(case)
    losses = []
    for step in range(4):
        losses.append(b.grad(env)[1])
        env.train_adam_device(0, 1e-3)
    print(f"surrogate loss {losses}")
    assert losses[-1] < losses[0], losses
    env.close()
    print("optimises ok")


def wrapper(opt):
    import torch.nn as nn
    from ft_grandprix_amd.net import NetSpec, value_from_torch
    from ft_grandprix_amd.vec import DeviceVecEnv
    from tests import collect_child as cc
    net = cc.driver_net(71)
    spec = NetSpec(net["layers"], **cc.fields(net))
    kw = dict(n_envs=8, n_rays=64, cars_per_env=1, roster=["agent"], max_episode_steps=50, scan_pool=4, scan_max_range=3.0, state=True, spawn_mode=1, seed=9)
    a = DeviceVecEnv("small-circle", nets={0: spec, 1: spec}, **kw)
    h = DeviceVecEnv("small-circle", nets={0: spec}, **kw)
    a.reset(); h.reset()
    torch.manual_seed(5)
    critic = nn.Sequential(nn.Linear(17, 32), nn.Tanh(), nn.Linear(32, 1))

    def refused(call, exc):
        try:
            call()
        except exc:
            return
        raise AssertionError("a bad trainer call was accepted")
    refused(lambda: a.train_begin(0), ValueError)                     # no value net
    a.set_value_net(0, critic); h.set_value_net(0, critic)
    a.set_population(1, torch.from_numpy(np.stack([spec.flat_params()] * 2)).to(a.device))
    a.set_value_net(1, critic)
    refused(lambda: a.train_begin(1), ValueError)                     # a population
    refused(lambda: a.env.train_begin(1), capi.FtgpError)
    refused(lambda: a.env.train_adam_device(0, 1e-3), capi.FtgpError)     # no trainer yet
    a.train_begin(0); h.train_begin(0)
    refused(lambda: a.train_begin(0), capi.FtgpError)                 # twice
    T, std = 4, (0.3, 0.1)
    gen = torch.Generator(device=a.device); gen.manual_seed(11)
    noise = torch.randn((T, 8, 1, 2), generator=gen, device=a.device)
    ra = a.collect(T, std=std, noise=noise, values=True)
    rh = h.collect(T, std=std, noise=noise, values=True)
    ga = torch.Generator(device=a.device); ga.manual_seed(3)
    stats = a.ppo_update(ra, epochs=2, minibatches=3, lr=1e-3, std=std, generator=ga)
    # the same calls by hand through capi
    gh = torch.Generator(device=a.device); gh.manual_seed(3)
    n = T * 8
    adv = rh.advantage
    mu = adv.mean(); var = ((adv - mu) ** 2).mean()
    w = torch.ones_like(adv); s = w.sum().clamp_min(1e-12)
    mu = (w * adv).sum() / s; var = (w * (adv - mu) ** 2).sum() / s
    adv = ((adv - mu) / (var.sqrt() + 1e-8)).contiguous()
    edges = [n * k // 3 for k in range(4)]
    hand = torch.zeros((6, 8), device=a.device)
    for ep in range(2):
        perm = torch.randperm(n, device=a.device, generator=gh).to(torch.int32)
        for k in range(3):
            h.env.train_grad_device(capi.train_batch(n, edges[k + 1] - edges[k], index=perm.data_ptr() + 4 * edges[k], inputs=rh.inputs.data_ptr(),
                                                     mean=rh.mean.data_ptr(), noise=rh.noise.data_ptr(), advantage=adv.data_ptr(), ret=rh.returns.data_ptr(),
                                                     std=std, clip=0.2, value_coef=0.5, stats=hand.data_ptr() + 32 * (ep * 3 + k)))
            h.env.train_adam_device(0, 1e-3)
        torch.cuda.synchronize()
    assert tuple(stats.shape) == (6, 8) and stats.dtype == torch.float32
    assert stats.cpu().numpy().tobytes() == hand.cpu().numpy().tobytes(), (stats, hand)
    assert np.isfinite(stats.cpu().numpy()).all() and (stats[:, 0].cpu().numpy() > 0).all()
    for got, want in ((a.env.net(0)[1], h.env.net(0)[1]), (a.env.get_value_net(0)[1], h.env.get_value_net(0)[1])):
        assert tm.flat(got).tobytes() == tm.flat(want).tobytes(), "ppo_update against the same calls by hand"
    assert tm.flat(a.env.net(0)[1]).tobytes() != spec.flat_params().tobytes(), "the parameters moved"
    assert a.env.train_get(0)[2] == 6
    # set_net_params keeps the trainer, set_net ends it
    a.set_net_params(0, torch.from_numpy(spec.flat_params()).to(a.device))
    a.set_value_params(0, torch.from_numpy(value_from_torch(critic).flat_params()).to(a.device))
    assert a.env.train_get(0)[2] == 6 and np.abs(a.env.train_get(0, capi.TRAIN_M)[0]).max() > 0
    # the device-side refusals: a host pointer, a short buffer
    host = np.zeros(n * 17, dtype=F)
    # (the check knows an allocation's extent from the runtime, and torch carves small tensors out of larger allocations: 12 MB is an
    # allocation of its own, and an address near its end has that much room and no more)
    own = torch.zeros(3 << 20, device=a.device)
    end = own.data_ptr() + 4 * (3 << 20)
    ok = dict(inputs=ra.inputs.data_ptr(), mean=ra.mean.data_ptr(), advantage=ra.advantage.data_ptr(), ret=ra.returns.data_ptr())
    for bad, word in ((dict(inputs=host.ctypes.data), "inputs"), (dict(advantage=end - 4 * (n - 1)), "advantage"), (dict(stats=end - 16), "stats")):
        try:
            a.env.train_grad_device(capi.train_batch(n, n, **{**ok, **bad}))
        except capi.FtgpError as x:
            assert x.code == ERR_ARG and word in str(x), str(x)
        else:
            raise AssertionError(f"a bad {word} was accepted")
    # every FTGP_ERR_ARG of the C entries themselves, on structs built past the binding's own checks: the code and the field's name
    import ctypes
    lib = a.env.lib

    def c_refused(entry, word, *args):
        rc = lib.fn(entry)(a.env.h, *args)
        assert rc == ERR_ARG and word in lib.last_error(), (entry, word, rc, lib.last_error())

    def batch(**over):
        b = capi.train_batch(n, n, **ok)
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(b, k)[v[0]] = v[1]
            else:
                setattr(b, k, v)
        return ctypes.byref(b)
    for over, word in ((dict(reserved=(0, 1)), "reserved"), (dict(reserved=(1, 1)), "reserved"), (dict(n_batch=0), "n_batch"), (dict(n_rows=0), "n_rows"),
                       (dict(first_row=1), "first_row"), (dict(first_row=-1), "first_row"), (dict(std=(0, float("nan"))), "std[0]"),
                       (dict(std=(1, 0.0)), "std[1]"), (dict(std=(1, float("inf"))), "std[1]"), (dict(clip=-0.5), "clip"), (dict(clip=float("nan")), "clip"),
                       (dict(value_coef=float("inf")), "value_coef"), (dict(value_coef=-1.0), "value_coef"), (dict(slot=7), "slot"), (dict(slot=-1), "slot")):
        c_refused("train_grad_device", word, batch(**over))
    for lr in (float("nan"), float("inf"), -1e-3):
        c_refused("train_adam_device", "lr", None, 0, lr)
    c_refused("train_adam_device", "slot", None, 4, 1e-3)
    for fields, word in ((dict(beta1=1.0), "beta1"), (dict(beta1=-0.1), "beta1"), (dict(beta2=float("nan")), "beta2"), (dict(beta2=1.5), "beta2"),
                         (dict(eps=0.0), "eps"), (dict(eps=float("inf")), "eps"), (dict(reserved=1), "reserved")):
        c_refused("train_begin", word, 0, ctypes.byref(capi.FtgpTrainDesc(**{**dict(beta1=0.9, beta2=0.999, eps=1e-8), **fields})))
    c_refused("train_begin", "desc", 0, None)
    c_refused("train_begin", "slot", 4, ctypes.byref(capi.train_desc()))
    c_refused("train_get", "what", 0, 5, None, None, None)
    c_refused("train_get", "what", 0, -1, None, None, None)
    c_refused("train_end", "slot", 4)
    assert a.env.train_get(0)[2] == 6, "the refused calls changed nothing"
    a.set_net(0, NetSpec(cc.driver_net(72, hidden=8)["layers"], **cc.fields(net)))         # another shape: the trainer ends (and the value net)
    refused(lambda: a.env.train_get(0), capi.FtgpError)
    refused(lambda: a.env.train_end(0), capi.FtgpError)
    h.train_end(0)
    refused(lambda: h.env.train_adam_device(0, 1e-3), capi.FtgpError)
    a.close(); h.close()
    print("wrapper ok")


def lifecycle(opt):
    """What ends with what on a network slot (include/ftgp.h), edge by edge through capi alone on 2 envs of 1 car and 36 rays: after every
    setter, what must be gone is refused with its code and its words, what must have survived reads back with the bits that went in, and
    slot 0 -- a policy, a value net and a trainer one Adam step old -- is untouched by everything done to slot 1.  Then each stream-ordered
    entry that needs no ftgp_device_io_config, as the first stream-ordered call of a fresh handle, on a stream of the caller's.
    (A slot cannot hold a population and a trainer at once -- either refuses the other --, so ftgp_set_net meets them in two steps.)"""
    lib, track = capi.load(), load_track("small-circle")
    rng = np.random.default_rng(23)
    N_IN, KW = 8, dict(pool=1, max_range=3.0, beam_first=4, n_beams=8)       # the drivers' window of 36 rays: [4, 32)

    def mlp(*widths):
        return [(rng.standard_normal((o, i)).astype(F), rng.standard_normal(o).astype(F)) for i, o in zip(widths[:-1], widths[1:])]

    def fresh():
        return capi.Env(lib, track, n_envs=2, cars_per_env=1, n_rays=36, spawn_mode=1, seed=3)

    def gone(call, code, *words):
        try:
            call()
        except capi.FtgpError as x:
            assert x.code == code and all(w in str(x) for w in words), (code, words, str(x))
        else:
            raise AssertionError(f"accepted: what should be refused with {code} {words}")

    def bits(what, got, want):
        cmod.assert_same_bits(tm.flat(got), tm.flat(want), what)

    env = fresh()

    def policy_is(what, slot, layers):
        bits(f"{what}: slot {slot}'s policy", env.net(slot)[1], layers)

    def value_is(what, slot, layers):
        bits(f"{what}: slot {slot}'s value net", env.get_value_net(slot)[1], layers)

    def no_trainer(slot):
        gone(lambda: env._call("train_get", slot, capi.TRAIN_GRAD, None, None, None), ERR_STATE, "train_get", "trainer")
        gone(lambda: env.train_adam_device(slot, 1e-3), ERR_STATE, "train_adam_device", "trainer")
        gone(lambda: env.train_end(slot), ERR_STATE, "train_end", "trainer")

    def no_value(slot, defined=True):
        gone(lambda: env._call("get_value_net", slot, None, None), ERR_STATE, "get_value_net", "value net")
        gone(lambda: env.train_begin(slot), ERR_STATE, "train_begin", "value net" if defined else "not defined")

    def no_population(slot):
        assert env.get_net_population(slot) == (0, None)
        gone(lambda: env.set_net_population_device(slot, 0, 0), ERR_STATE, "set_net_population_device", "population")
        gone(lambda: env.get_net_population(slot, 0), ERR_STATE, "get_net_population", "population")

    # slot 0: everything a slot can hold beside a population, and one Adam step on a zero gradient (t = 1, the parameters as they were)
    P0, V0 = mlp(N_IN, 4, 2), mlp(N_IN, 4, 1)
    env.set_net(0, P0, **KW); env.set_value_net(0, V0); env.train_begin(0); env.train_adam_device(0, 1e-3)

    def slot0_untouched(what):
        policy_is(what, 0, P0); value_is(what, 0, V0)
        pol, val, t = env.train_get(0, capi.TRAIN_M)
        assert t == 1 and not pol.any() and not val.any(), (what, t)
        assert env.get_net_population(0) == (0, None), what
    slot0_untouched("at the start")

    P1, V1, P1b, V1b = mlp(N_IN, 4, 2), mlp(N_IN, 4, 1), mlp(N_IN, 5, 2), mlp(N_IN, 3, 1)
    members, env_member = np.stack([tm.flat(mlp(N_IN, 4, 2)) for _ in range(2)]), np.array([1, 0], dtype=np.int32)

    def population_is(what):
        n, m = env.get_net_population(1)
        assert n == 2 and (m == env_member).all(), (what, n, m)
        for k in range(2):
            cmod.assert_same_bits(env.get_net_population(1, k), members[k], f"{what}: member {k}")
        gone(lambda: env.set_net_device(1, 0), ERR_STATE, "set_net_device", "population", "member")

    # ftgp_set_net_population with members on a slot with a value net and a trainer: the trainer is gone, the value net stays
    env.set_net(1, P1, **KW); env.set_value_net(1, V1); env.train_begin(1)
    assert env.train_get(1)[2] == 0
    env.set_net_population(1, members, env_member)
    what = "a population installed"
    no_trainer(1); population_is(what); policy_is(what, 1, P1); value_is(what, 1, V1); slot0_untouched(what)
    gone(lambda: env.train_begin(1), ERR_STATE, "train_begin", "population", "member")
    # ftgp_set_net with a new description on a slot with a population and a value net: both are gone, the slot is defined
    env.set_net(1, P1b, **KW)
    what = "set_net on a population and a value net"
    policy_is(what, 1, P1b); no_population(1); no_value(1); no_trainer(1); slot0_untouched(what)
    # ... and on a slot with a value net and a trainer
    env.set_value_net(1, V1b); env.train_begin(1)
    env.set_net(1, P1, **KW)
    what = "set_net on a value net and a trainer"
    policy_is(what, 1, P1); no_population(1); no_value(1); no_trainer(1); slot0_untouched(what)
    # ftgp_set_net(NULL): the slot is undefined
    env.set_net(1, None)
    for call, entry in ((lambda: env.net(1), "get_net"), (lambda: env.net_frame(1), "get_net_frame"), (lambda: env.net_rivals(1), "get_net_rivals"),
                        (lambda: env.get_net_population(1), "get_net_population"), (lambda: env.set_value_net(1, V1), "get_net"),
                        (lambda: env.set_net_population(1, None), "set_net_population"), (lambda: env.set_net_device(1, 0), "set_net_device")):
        gone(call, ERR_STATE, entry, "slot 1", "not defined")
    no_value(1, defined=False); no_trainer(1); slot0_untouched("set_net(NULL)")
    gone(lambda: env.rollout("net1", 1), ERR_STATE, "slot 1", "not defined")
    # ftgp_set_net_population with 0 members: the single set is in force again, bit for bit, and the value net stays
    env.set_net(1, P1, **KW); env.set_value_net(1, V1); env.set_net_population(1, members, env_member)
    population_is("a population again")
    env.set_net_population(1, None)
    what = "the population removed"
    no_population(1); policy_is(what, 1, P1); value_is(what, 1, V1); no_trainer(1); slot0_untouched(what)
    same = dev(tm.flat(P1))
    env.set_net_device(1, same.data_ptr()); torch.cuda.synchronize()        # accepted again: no population
    policy_is(what + ", set_net_device", 1, P1)
    # ftgp_set_value_net with a description, then with NULL, on a slot with a trainer: the trainer is gone each time, the policy stays
    env.train_begin(1)
    env.set_value_net(1, V1b)
    what = "set_value_net on a trainer"
    no_trainer(1); policy_is(what, 1, P1); value_is(what, 1, V1b); no_population(1); slot0_untouched(what)
    env.train_begin(1)
    env.set_value_net(1, None)
    what = "set_value_net(NULL) on a trainer"
    no_trainer(1); no_value(1); policy_is(what, 1, P1); no_population(1); slot0_untouched(what)
    # ftgp_train_end: both nets stay
    env.set_value_net(1, V1); env.train_begin(1)
    env.train_end(1)
    what = "train_end"
    no_trainer(1); policy_is(what, 1, P1); value_is(what, 1, V1); no_population(1); slot0_untouched(what)
    env.train_begin(1)                                           # ... and a new trainer starts at t = 0
    assert env.train_get(1)[2] == 0
    env.close()

    # each stream-ordered entry as a fresh handle's first stream-ordered call, on a stream of the caller's
    stream = torch.cuda.Stream()
    new = dev(tm.flat(P1))
    torch.cuda.synchronize()
    env = fresh(); env.set_net(0, P0, **KW)
    env.set_net_device(0, new.data_ptr(), stream=stream.cuda_stream); stream.synchronize()
    policy_is("set_net_device first", 0, P1)
    env.close()
    new = dev(tm.flat(V1))
    torch.cuda.synchronize()
    env = fresh(); env.set_net(0, P0, **KW); env.set_value_net(0, V0)
    env.set_value_net_device(0, new.data_ptr(), stream=stream.cuda_stream); stream.synchronize()
    value_is("set_value_net_device first", 0, V1); policy_is("set_value_net_device first", 0, P0)
    env.close()
    env = fresh(); env.set_net(0, P0, **KW); env.set_value_net(0, V0); env.train_begin(0)
    env.train_adam_device(0, 1e-3, stream=stream.cuda_stream); stream.synchronize()
    assert env.train_get(0)[2] == 1
    policy_is("train_adam_device first", 0, P0); value_is("train_adam_device first", 0, V0)      # (a zero gradient moves nothing)
    env.close()
    env = fresh()
    n = env.env_state_bytes() * 2
    rows, again = (torch.full((n,), 0xAA, dtype=torch.uint8, device=DEV) for _ in range(2))
    torch.cuda.synchronize()
    env.save_envs_device(rows.data_ptr(), 2, stream=stream.cuda_stream); stream.synchronize()
    env.save_envs_device(again.data_ptr(), 2, stream=stream.cuda_stream)
    env.load_envs_device(rows.data_ptr(), 2, stream=stream.cuda_stream); stream.synchronize()
    assert (rows.cpu().numpy() != 0xAA).any() and rows.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() and env.env_state_rejected() == 0
    env.close()
    print("lifecycle ok")


def ppo_tool(opt):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ppo.py"), "--device-update", "--envs", "64", "--iterations", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 2, r.stdout
    for row in rows:
        assert row["update"] == "device" and np.isfinite([row["loss_pi"], row["loss_v"]]).all(), row
    print("ppo tool ok")


if __name__ == "__main__":
    scenario = sys.argv[1]
    options = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
    {"gradient": gradient, "turns": turns, "collected": collected, "adam": adam, "determinism": determinism, "guards": guards, "optimises": optimises,
     "wrapper": wrapper, "lifecycle": lifecycle, "ppo_tool": ppo_tool}[scenario](options)
