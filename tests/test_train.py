"""Training on the device (include/ftgp.h "Training on the device": ftgp_train_begin, ftgp_train_end, ftgp_train_grad_device,
ftgp_train_adam_device, ftgp_train_get; ft_grandprix_amd/vec.py: DeviceVecEnv.train_begin, ppo_update).

CPU: the binding and the header; the argument checks that need no device; the shipped Adam element step (csrc/ftgp_net.h, compiled for
the host by tools/train_check.cpp, also under the address and undefined-behaviour sanitizers) against the numpy model of the header's
text (tests/train_model.py), bit for bit; the model's gradient against central differences of the model's loss in binary64.

GPU: every scenario runs in a fresh child process (tests/train_child.py), one at a time, each under a time limit (tests/children.py).
The forward pass and Adam are compared to the bit; the gradient and the stats within 4 * rel_ref of the binary64 model, rel_ref being
what the same model in binary32, rows accumulated one after the other, loses against it -- the factor covers another order of the sums
and the device's exp.  Where a batch has more tiles than workgroups, a workgroup adds several tiles into its partial sums: a batch that
is zeros but for one or two tiles is compared exactly with a call on those tiles' rows alone (`turns`).  The CPU side restates the
host's LDS row rule (train_model.row_layout) and pins the tile size and the number of tiles of every case that is there for a path.
"""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import children
from tests import collect_model as cmod
from tests import train_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "train_child.py")

run_child = functools.partial(children.run_child, CHILD, timeout=300)
F = np.float32
NEW = ("train_begin", "train_end", "train_grad_device", "train_adam_device", "train_get")


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_header_binding_and_export_agree():
    from ft_grandprix_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "ftgp.h")).read()
    for name in NEW:
        assert name in capi.API_SYMBOLS and lib.has(name) and lib.fn(name).argtypes is not None, name
        assert re.search(r"\bint ftgp_%s\(FtgpEnv \*env" % name, header), name
    assert "#define FTGP_ABI_VERSION 5" in header and capi.ABI_VERSION == 5
    assert ctypes.sizeof(capi.FtgpCollect) == 120
    assert "#define FTGP_TRAIN_STATS 8" in header and capi.TRAIN_STATS == 8
    assert (capi.TRAIN_GRAD, capi.TRAIN_M, capi.TRAIN_V, capi.TRAIN_RAW_GRAD, capi.TRAIN_RAW_PARAMS) == (0, 1, 2, 3, 4)
    for k, name in enumerate(("GRAD", "M", "V", "RAW_GRAD", "RAW_PARAMS")):
        assert re.search(r"#define FTGP_TRAIN_%s\s+%d\b" % (name, k), header)
    D = capi.FtgpTrainDesc
    assert ctypes.sizeof(D) == 16 and (D.beta1.offset, D.beta2.offset, D.eps.offset, D.reserved.offset) == (0, 4, 8, 12)
    # pointer, 4 x int32, 7 pointers, 4 x float, 3 pointers, int32[2]
    B = capi.FtgpTrainBatch
    assert ctypes.sizeof(B) == 8 + 16 + 7 * 8 + 16 + 3 * 8 + 8 == 128
    names = ("stream", "slot", "n_rows", "n_batch", "first_row", "index", "inputs", "mean", "noise", "advantage", "ret", "weight", "std", "clip",
             "value_coef", "stats", "new_mean", "new_value", "reserved")
    assert [getattr(B, n).offset for n in names] == [0, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92, 96, 104, 112, 120]
    for struct, fields in (("FtgpTrainDesc", ("beta1", "beta2", "eps", "reserved")), ("FtgpTrainBatch", names)):
        body = header.split("typedef struct %s {" % struct)[1].split("} %s;" % struct)[0]
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S).replace("*", " ").replace(",", " ").replace(";", " ").replace("[", " ")
        words = body.split()
        order = [words.index(n) for n in fields]
        assert order == sorted(order), (struct, order)                  # the fields, in the binding's order
    for name in NEW:
        assert callable(getattr(capi.Env, name))
    from ft_grandprix_amd import vec
    for name in ("train_begin", "train_end", "ppo_update"):
        assert callable(getattr(vec.DeviceVecEnv, name))


def test_null_handles_are_refused_without_a_device():
    from ft_grandprix_amd import capi
    lib = capi.load()
    d = capi.train_desc()
    b = capi.train_batch(8, 4, inputs=4096, mean=4096, advantage=4096, ret=4096)
    assert lib.fn("train_begin")(None, 0, d) == -1 and "null" in lib.last_error()
    assert lib.fn("train_end")(None, 0) == -1 and "null" in lib.last_error()
    assert lib.fn("train_grad_device")(None, b) == -1 and "null" in lib.last_error()
    assert lib.fn("train_grad_device")(None, None) == -1
    assert lib.fn("train_adam_device")(None, None, 0, 1e-3) == -1 and "null" in lib.last_error()
    assert lib.fn("train_get")(None, 0, 0, None, None, None) == -1 and "null" in lib.last_error()


@pytest.mark.parametrize("bad", [dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(betas=(float("nan"), 0.9)), dict(betas=(0.9,)), dict(betas=0.9),
                                 dict(eps=0.0), dict(eps=-1e-8), dict(eps=float("inf")), dict(eps="x"), dict(betas=(0.9, float("inf")))])
def test_train_desc_refuses_bad_fields_before_a_handle_is_touched(bad):
    from ft_grandprix_amd import capi
    with pytest.raises(ValueError):
        capi.train_desc(**bad)


def test_train_desc_fills_the_fields():
    from ft_grandprix_amd import capi
    d = capi.train_desc()
    assert (d.beta1, d.beta2, d.eps, d.reserved) == (float(F(0.9)), float(F(0.999)), float(F(1e-8)), 0)
    d = capi.train_desc((0.0, 0.5), 1e-3)
    assert (d.beta1, d.beta2, d.eps) == (0.0, 0.5, float(F(1e-3)))


@pytest.mark.parametrize("bad", [dict(n_rows=0), dict(n_batch=0), dict(n_batch=9), dict(first_row=-1), dict(first_row=5), dict(n_rows=True),
                                 dict(std=(0.0, 0.1)), dict(std=(0.3, -0.1)), dict(std=(0.3, float("nan"))), dict(std=(0.3, float("inf"))), dict(std=0.3),
                                 dict(clip=-0.1), dict(clip=float("nan")), dict(clip=float("inf")), dict(value_coef=-1.0), dict(value_coef=float("nan")),
                                 dict(slot=4), dict(slot=-1), dict(inputs=0), dict(mean=0), dict(advantage=0), dict(ret=0)])
def test_train_batch_refuses_bad_fields_before_a_handle_is_touched(bad):
    from ft_grandprix_amd import capi
    kw = dict(n_rows=8, n_batch=4, inputs=4096, mean=4096, advantage=4096, ret=4096, std=(0.3, 0.1))
    with pytest.raises(ValueError):
        capi.train_batch(**{**kw, **bad})


def test_train_batch_fills_the_fields():
    from ft_grandprix_amd import capi
    b = capi.train_batch(8, 4, first_row=4, inputs=4096, mean=8192, advantage=12288, ret=16384, std=(0.3, 0.1), clip=0.25, value_coef=1.0)
    assert (b.slot, b.n_rows, b.n_batch, b.first_row, b.index, b.noise, b.weight, b.stats, b.new_mean, b.new_value) == (0, 8, 4, 4) + (None,) * 6
    assert (b.inputs, b.mean, b.advantage, b.ret, list(b.std), b.clip, b.value_coef) == (4096, 8192, 12288, 16384, [float(F(0.3)), float(F(0.1))], 0.25, 1.0)
    assert list(b.reserved) == [0, 0]
    b = capi.train_batch(8, 20, index=4096, first_row=7, inputs=4096, mean=4096, advantage=4096, ret=4096)      # with an index: any B, first_row unused
    assert (b.n_batch, b.first_row, b.index) == (20, 0, 4096)


def test_device_vec_env_checks_its_train_arguments_first():
    """DeviceVecEnv.train_begin and ppo_update on an object that holds no handle: the refusals come before anything of the env is used."""
    from ft_grandprix_amd import vec
    env = object.__new__(vec.DeviceVecEnv)
    env._nets, env._pops, env._vnets = {0: (((17, 2),), None), 1: (((17, 2),), None)}, {1: (2, None)}, {1: ((17, 1), None)}
    for kw in (dict(slot=0), dict(slot=1), dict(slot=2), dict(slot=0, betas=(1.0, 0.9)), dict(slot=0, eps=0.0)):
        with pytest.raises(ValueError):
            env.train_begin(**kw)
    for kw in (dict(epochs=0), dict(minibatches=0), dict(roll=None), dict(roll=vec.Rollout(*([None] * 6)))):
        with pytest.raises(ValueError):
            env.ppo_update(**{"roll": None, **kw})


# ---- Adam: the shipped element step against the model
def sanitizers_available(cxx, flags, tmp):
    """Whether the host compiler builds and runs an empty program with the sanitizer flags: decided before the code under test is touched."""
    src = tmp / "empty.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp / "empty")
    if subprocess.run([cxx, *flags, str(src), "-o", exe], capture_output=True, text=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True, text=True).returncode == 0


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("train")
    out = str(tmp / f"train_check_{request.param}")
    flags = ["-O2", "-ffp-contract=off", "-std=c++17"]
    if request.param == "sanitized":
        # (the runtimes linked statically where the compiler knows the switches: the program then needs nothing of its environment)
        version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]          # (clang links them statically anyway)
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static]
        if not sanitizers_available(cxx, flags, tmp):
            pytest.skip("the host compiler has no sanitizer runtimes (an empty program does not build and run with them)")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "train_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_harness(harness, tmp_path, name, p, m, v, g, t, betas=(0.9, 0.999), eps=1e-8, lr=3e-4):
    """(scalars, p, m, v) of tools/train_check after one step."""
    p, m, v, g = (np.ascontiguousarray(a, dtype=F) for a in (p, m, v, g))
    src, out = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    with open(src, "wb") as f:
        np.array([p.size], dtype=np.int32).tofile(f)
        np.array([t], dtype=np.int64).tofile(f)
        np.array([betas[0], betas[1], eps, lr], dtype=F).tofile(f)
        for a in (p, m, v, g):
            a.tofile(f)
    r = subprocess.run([harness, str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=F)
    n = p.size
    return got[:6], got[6:6 + n], got[6 + n:6 + 2 * n], got[6 + 2 * n:]


def adam_cases():
    rng = np.random.default_rng(4)
    n = 257
    r = lambda s=1.0: (s * rng.standard_normal(n)).astype(F)          # noqa: E731
    pos = lambda s=1.0: np.abs(r(s))                                  # noqa: E731
    return {"random": (r(), r(0.1), pos(0.01), r(0.1)),
            "g_zero": (r(), r(0.1), pos(0.01), np.zeros(n, dtype=F)),
            "v_zero": (r(), r(0.1), np.zeros(n, dtype=F), r(0.1)),
            "all_zero": (r(), np.zeros(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=F)),
            "huge_g": (r(), r(0.1), pos(0.01), r(1e25)),
            "tiny_g": (r(), r(1e-30), pos(1e-38), r(1e-30))}


@pytest.mark.parametrize("t", [1, 10 ** 4])
@pytest.mark.parametrize("case", sorted(adam_cases()))
def test_adam_harness_equals_the_model(harness, tmp_path, case, t):
    p, m, v, g = adam_cases()[case]
    sc, p1, m1, v1 = run_harness(harness, tmp_path, f"{case}_{t}", p, m, v, g, t)
    want_sc = tm.adam_scalars(0.9, 0.999, 3e-4, t)
    cmod.assert_same_bits(sc, np.array(want_sc, dtype=F), f"{case}, t = {t}: the scalars")
    wp, wm, wv = tm.adam_step(p, m, v, g, want_sc, 1e-8)
    cmod.assert_same_bits(p1, wp, f"{case}, t = {t}: p"); cmod.assert_same_bits(m1, wm, f"{case}, t = {t}: m"); cmod.assert_same_bits(v1, wv, f"{case}, t = {t}: v")
    if case == "all_zero":                                            # what keeps the library layout's padding: p - a * (0 / eps) = p
        cmod.assert_same_bits(p1, p, "g = m = v = 0 leaves p")
        assert not m1.any() and not v1.any()
    if case == "huge_g":
        assert np.isinf(v1).any()                                     # g * g overflows: d is infinite and p stays
    if t == 10 ** 4:
        assert sc[4] == F(3e-4) and abs(float(sc[5]) - 1.0 / np.sqrt(1.0 - 0.999 ** 1e4)) < 1e-7


def test_an_element_written_out_by_hand(harness, tmp_path):
    """beta1 = 1/2, beta2 = 3/4, lr = 1/4, t = 1, m = v = 0, g = 4, p = 1: every scalar is a power of two (a = 1/2, r = 2), m = 2, v = 4,
    d = 2 * 2 + eps.  With eps = 2^-10 the quotient rounds once and the fused last step once more; with eps = 4 every step is exact:
    p = 1 - (1/2) * (2 / 8) = 0.875."""
    sc, p1, m1, v1 = run_harness(harness, tmp_path, "hand", [1.0], [0.0], [0.0], [4.0], 1, betas=(0.5, 0.75), eps=2.0 ** -10, lr=0.25)
    np.testing.assert_array_equal(sc, np.array([0.5, 0.75, 0.5, 0.25, 0.5, 2.0], dtype=F))
    assert m1[0] == 2.0 and v1[0] == 4.0
    d = F(4.0 + 2.0 ** -10)                                           # exact in binary32
    want = F(np.float64(1.0) - 0.5 * np.float64(F(F(2.0) / d)))       # fmaf: one rounding of the exact 1 - q/2
    assert p1[0] == want
    wp, wm, wv = tm.adam_step([1.0], [0.0], [0.0], [4.0], tm.adam_scalars(0.5, 0.75, 0.25, 1), 2.0 ** -10)
    assert (wp[0], wm[0], wv[0]) == (want, 2.0, 4.0)
    # and one whose every step is exact: eps = 0 is refused by the library, so d = 4 + 4 = 8 with eps = 4: p = 1 - (1/2) * (2 / 8) = 0.875
    _, p2, _, _ = run_harness(harness, tmp_path, "hand2", [1.0], [0.0], [0.0], [4.0], 1, betas=(0.5, 0.75), eps=4.0, lr=0.25)
    assert p2[0] == F(0.875)


# ---- the model's calculus
def small_case(hidden, out_act, seed):
    rng = np.random.default_rng(seed)
    n = 24
    policy = dict(layers=tm.random_layers(rng, (5, 4, 2)), hidden_act=hidden, out_act=out_act, out_scale=(1.5, 0.6), out_offset=(1.0, 0.0))
    value = dict(layers=tm.random_layers(rng, (5, 4, 1)), hidden_act=hidden, out_act="identity", out_scale=2.0, out_offset=0.25)
    inputs = rng.uniform(-1, 1, (n, 5)).astype(F)
    t = tm.loss_terms(dict(policy=policy, value=value, inputs=inputs, rows=np.arange(n), weight=None, noise=None, mean=np.zeros((n, 2), dtype=F),
                           advantage=np.zeros(n, dtype=F), ret=np.zeros(n, dtype=F), std=(1.0, 1.0), clip=0.2, value_coef=0.5))
    # unclipped rows: the recorded mean is the policy's own, moved a little, so that rho stays inside the clip
    mean = (t["m"] + 0.01 * rng.standard_normal((n, 2))).astype(F)
    return dict(policy=policy, value=value, inputs=inputs, rows=np.arange(n), weight=rng.uniform(0.5, 1.5, n).astype(F),
                noise=(0.5 * rng.standard_normal((n, 2))).astype(F), mean=mean, advantage=rng.standard_normal(n).astype(F),
                ret=rng.standard_normal(n).astype(F), std=(F(0.3), F(0.1)), clip=F(0.2), value_coef=F(0.5))


@pytest.mark.parametrize("hidden,out_act", [("tanh", "tanh"), ("relu", "identity")])
def test_the_models_gradient_is_the_derivative_of_the_models_loss(hidden, out_act):
    """5 -> 4 -> 2 / 5 -> 4 -> 1 on unclipped rows: the chain rule written out against central differences of L in binary64."""
    case = small_case(hidden, out_act, 3)
    t = tm.loss_terms(case)
    assert t["active"].all() and (np.abs(t["rho"] - 1) < 0.19).all()
    if hidden == "relu":
        assert all((np.abs(a) > 1e-3).all() for a in t["ppre"][:-1] + t["vpre"][:-1])
    gp, gv, _ = tm.loss_and_grad(case)
    layers = [[(W.astype(np.float64), b.astype(np.float64)) for W, b in case[k]["layers"]] for k in ("policy", "value")]
    h = 1e-6
    for which, grads in enumerate((gp, gv)):
        for l, (dW, db) in enumerate(grads):
            for part, g in enumerate((dW, db)):
                num = np.zeros_like(g)
                for idx in np.ndindex(*g.shape):
                    a = layers[which][l][part]
                    keep = a[idx]
                    a[idx] = keep + h; up = tm.loss(case, layers)
                    a[idx] = keep - h; down = tm.loss(case, layers)
                    a[idx] = keep
                    num[idx] = (up - down) / (2 * h)
                assert np.abs(num - g).max() <= 1e-7 * max(1.0, np.abs(g).max()), (which, l, part, np.abs(num - g).max())
                assert np.abs(g).max() > 1e-3


def test_the_gradient_cases_meet_their_conditions():
    for name in tm.CASES:
        case = tm.make_case(name)
        if name not in tm.LOOSE:
            assert tm.conditions(case) is None
        assert len(case["rows"]) == tm.CASES[name][6]
    a = tm.make_case("a")
    assert np.unique(a["rows"]).size < len(a["rows"]) and (a["weight"] == 0).any()
    for name in ("turns32", "turns16"):
        c = tm.make_case(name)
        assert np.unique(c["rows"]).size < len(c["rows"]) and (c["weight"] == 0).any()


def test_row_layout_written_out_by_hand():
    """The host's row rule on shapes added up by hand.  d: 33 -> 65 -> 2 and -> 1: 36 + 68 + 4 = 108 floats of outputs, two delta
    buffers of 128: 364 = 4 * 91, odd.  a: 88 + 64 + 64 + 4 = 220, + 2 * 64 = 348 = 4 * 87.  c: 256 + 3 * 128 + 4 = 644, + 256 = 900
    = 4 * 225; 32 * 900 * 4 bytes are more than 63 KiB.  A net of (8, 2) and (8, 1): 12 + 128 = 140 = 4 * 35."""
    assert tm.row_layout((33, 65, 2), (33, 65, 1)) == (364, 32)
    assert tm.row_layout((85, 64, 64, 2), (85, 64, 64, 1)) == (348, 32)
    assert tm.row_layout((256, 128, 128, 128, 2), (256, 128, 128, 128, 1)) == (900, 16)
    assert tm.row_layout((8, 2), (8, 1)) == (140, 32)
    # the bump: 4 + 4 + 128 = 136 = 4 * 34, even: four more
    assert tm.row_layout((4, 2), (4, 1)) == (140, 32)
    # the longer net sets the outputs, the widest layer of either the delta buffers: (33, 2) against (33, 100, 7, 33, 1)
    # (36 + 100 + 8 + 36 + 4 = 184, + 2 * 128 = 440 = 4 * 110, even: 444)
    assert tm.row_layout((33, 2), (33, 100, 7, 33, 1)) == (444, 32)
    assert tm.row_layout((33, 100, 7, 33, 2), (33, 1)) == (444, 32)


def test_the_gradient_cases_take_the_paths_they_are_meant_to():
    """The tile size and the number of tiles of the cases that are there for a path of the launch: a change to a case cannot move it off
    its path unseen."""
    rows = {name: tm.row_layout(*tm.case_widths(name))[1] for name in tm.CASES}
    floats = {name: tm.row_layout(*tm.case_widths(name))[0] for name in tm.CASES}
    assert rows["turns32"] == 32 and rows["edge32"] == 32 and rows["mixed"] == 32 and rows["mixed2"] == 32
    assert rows["turns16"] == 16 and rows["edge16"] == 16 and rows["c"] == 16
    # more tiles than workgroups, by two: workgroups 0 and 1 take a second tile, and the last tile is ragged
    for name in ("turns32", "turns16"):
        assert tm.n_tiles(name) == tm.MAX_WG + 2 and tm.CASES[name][6] % rows[name] != 0
    assert all(tm.n_tiles(name) <= tm.MAX_WG for name in tm.CASES if not name.startswith("turns"))
    # the edge of the tile-size rule: the largest row that takes 32 rows, and the next one (rows grow by 8 floats: an odd number of float4)
    assert floats["edge32"] == 500 and 32 * 500 * 4 <= 63 * 1024 < 32 * 508 * 4 and floats["edge16"] == 508
    # widths that are no multiple of 8 into the input delta (layers l > 0), a bias row inside a 32-row tile of k, nets of unlike shape
    dx_widths = {n for name in tm.CASES for w in tm.case_widths(name) for n in w[2:]}
    assert {7, 31, 33, 65, 97, 100} <= {n for name in ("mixed", "mixed2", "edge32") for w in tm.case_widths(name) for n in w[1:-1]}
    assert {1, 2, 7, 33, 64, 65, 97, 128} <= dx_widths
    assert {7, 31, 97, 100} <= {n for name in ("mixed", "mixed2") for w in tm.case_widths(name) for n in w[:-1]}
    for name in ("mixed", "mixed2"):
        pw, vw = tm.case_widths(name)
        assert len(pw) != len(vw) and max(pw[1:]) != max(vw[1:])
    # uneven: at layer 1 the weight gradient has (n_in + 1 tiles of 32) x (ld / 32) = 3 x 2 tiles, no multiple of the four waves; the
    # delta it reads is the second buffer (the buffers alternate from the last layer down), the one it writes is 128 columns wide
    n_in, n_out = tm.case_widths("uneven")[0][1:3]
    ld = lambda n: (n + 63) & ~63                                     # noqa: E731
    assert len(tm.case_widths("uneven")[0]) == 4 and ((n_in + 1 + 31) // 32) * (ld(n_out) // 32) % 4 != 0 and ld(n_in) == 128 and ld(n_out) == 64
    assert rows["uneven"] == 32


@pytest.mark.parametrize("name", ["turns32", "turns16"])
def test_the_turns_scenario_makes_no_nan_of_its_own(name):
    """tests/train_child.py `turns` gives most rows a weight of 0.  0 * infinity is a NaN, so every row of the buffers -- any of them may
    be named by an index -- has a finite ratio in the binary32 model, |logp - logq| < 80 (exp overflows binary32 at 88.7), and a finite
    value; the live rows are distinct, the dead ones are the rest, and only the live ones have a weight."""
    case = tm.make_case(name)
    span, finite = tm.ratio_span(case)
    assert finite and span < 80.0, (span, finite)
    R = tm.row_layout(*tm.case_widths(name))[1]
    tail = tm.turns_tail(name)
    assert 0 < tail < R
    live, dead, weight = tm.turns_rows(case, R, tail)
    assert live.size == 2 * R and np.unique(live).size == 2 * R and not np.intersect1d(live, dead).size and live.size + dead.size == case["n_rows"]
    assert (weight[live] >= 0.5).all() and not weight[dead].any() and np.isfinite(case["advantage"]).all() and np.isfinite(case["ret"]).all()
    index = tm.turns_index(dead, 5 * R, [(2 * R, live[:R])])
    assert index.dtype == np.int32 and (index[2 * R:3 * R] == live[:R]).all() and np.isin(np.delete(index, np.s_[2 * R:3 * R]), dead).all()
    # the clip leaves live rows free in each live tile: their gradient is not a zero
    t = tm.loss_terms(dict(case, rows=live, weight=weight))
    assert t["active"][R:].any() and t["active"][:tail].any()


def test_the_case_without_noise_meets_what_conditions_it_can():
    """noise = None: logq = 0 and rho = exp(logp) <= 1, so the clip cannot bind above 1 + clip for any seed; every other condition is
    asked as of the other cases (the clip binds below on 5 % of the weighted rows, 40 % are free, no row at an edge)."""
    case = tm.make_case("d", with_noise=False)
    assert case["noise"] is None and tm.conditions(case, high_side=False) is None
    assert "binds" in tm.conditions(case)                             # (the full conditions do name the high side)
    assert tm.loss_terms(case)["rho"].max() <= 1.0
    with_noise = tm.make_case("d")
    assert with_noise["noise"] is not None and tm.conditions(with_noise) is None


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_gradient_and_forward(case):
    """a: 85 -> 64 -> 64 at 517 rows through an index with repeats and zero weights; b: 1 -> 3, relu, 63 rows; c: 256 -> 128 x 3, 300
    rows from first_row 27 (tiles of 16 rows); d: hidden 65 (padding inside ld = 128), 257 rows; e: one-layer nets at 1 and at 64 rows.
    turns32: 17 -> 8, 8229 rows through an index: 258 tiles of 32 rows on 256 workgroups, so workgroups 0 and 1 take a second tile, the
    last one of 5 rows; turns16: 256 -> 128, 4115 rows: 258 tiles of 16 (rel_ref grows with the rows added up, to about 4e-6: these two are
    coarse, the sharp check of a second turn is test_a_tiles_share_does_not_depend_on_whose_turn_it_is).  mixed: a policy 33 -> 31 -> 97
    -> 2 next to a critic 33 -> 64 -> 1, relu; mixed2: a one-layer policy next to a critic 33 -> 100 -> 7 -> 33 -> 1 -- the nets share the
    LDS row, and widths that are no multiple of 8 go through the input delta, bias rows inside a 32-row tile of k through the weight
    gradient.  edge32 / edge16: 104 and 108 -> 65 -> 65: LDS rows of 500 and 508 floats, the largest that takes tiles of 32 rows (64000
    bytes) and the first that takes 16.  uneven: 33 -> 80 -> 24: waves that finish the middle layer's weight gradient early write the next
    delta while the others still read this one.
    Each case also reads the gradient, and after an Adam step the parameters, as raw library-layout memory: the padding is zero bits.
    stats [0], [2] and [4] (S, the value loss, the clipped fraction) are also compared to the bit with sums in the order the header
    gives -- a tile's rows, a workgroup's tiles, the workgroups -- S in binary32, the other two carried in binary64 and rounded once
    (tm.ordered_stats).
    (turns32 is the case that found the stats' sums wanting: added up in binary32 in that order, 8229 rows left stats [2] and [4] at
    4.0e-7 and 5.5e-7 of their scale, 9.27 times rel_ref = 5.92e-8, where 4 are allowed; the device now carries them in binary64.)"""
    assert f"gradient {case} ok" in run_child("gradient", only=case)


@pytest.mark.gpu
def test_gradient_without_noise():
    """Case d with noise = NULL (n = 0, logq = 0), in the model and in the call: the same criterion."""
    assert "gradient d without noise ok" in run_child("gradient", only="d", noise=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case,rows", [("turns32", 32), ("turns16", 16)])
def test_a_tiles_share_does_not_depend_on_whose_turn_it_is(case, rows):
    """All weights 0 but for one or two tiles' rows; every comparison exact (values: +0 and -0 may differ), against a call on the live
    rows alone (one tile, one workgroup).  258 tiles with the live one at 0, 255 (first turns), 256 (the second turn of workgroup 0) and
    257 (ragged); 769 tiles with the live one at 512 (a third turn behind a second turn of zeros); tiles 3 and 259 live, both workgroup
    3's, against a call of those two tiles on two workgroups; row numbers -1 and n_rows inside the live tile of a second turn; and a
    call with stats, new_mean and new_value NULL.  new_mean and new_value of every batch position to the bit against the model."""
    assert f"turns {case} ok" in run_child("turns", only=case, rows=rows)


@pytest.mark.gpu
def test_a_collected_rollout_with_unchanged_parameters():
    assert "collected ok" in run_child("collected")


@pytest.mark.gpu
def test_adam_to_the_bit():
    assert "adam ok" in run_child("adam")


@pytest.mark.gpu
def test_determinism():
    assert "determinism ok" in run_child("determinism")


@pytest.mark.gpu
def test_guards():
    assert "guards ok" in run_child("guards")


@pytest.mark.gpu
def test_it_optimises():
    assert "optimises ok" in run_child("optimises")


@pytest.mark.gpu
def test_device_vec_env_ppo_update():
    assert "wrapper ok" in run_child("wrapper")


@pytest.mark.gpu
def test_what_ends_with_what_on_a_slot():
    """ftgp_set_net, ftgp_set_net_population, ftgp_set_value_net and ftgp_train_end at every edge of a slot's lifetime rules; the
    stream-ordered setters as a handle's first stream-ordered call."""
    assert "lifecycle ok" in run_child("lifecycle")


@pytest.mark.gpu
def test_the_ppo_tool_with_the_device_update():
    assert "ppo tool ok" in run_child("ppo_tool")
