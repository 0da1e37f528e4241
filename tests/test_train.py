"""Training on the device (include/ftgp.h "Training on the device": ftgp_train_begin, ftgp_train_end, ftgp_train_grad_device,
ftgp_train_adam_device, ftgp_train_get; ft_grandprix_amd/vec.py: DeviceVecEnv.train_begin, ppo_update).

CPU: the binding and the header; the argument checks that need no device; the shipped Adam element step (csrc/ftgp_net.h, compiled for
the host by tools/train_check.cpp, also under the address and undefined-behaviour sanitizers) against the numpy model of the header's
text (tests/train_model.py), bit for bit; the model's gradient against central differences of the model's loss in binary64.

GPU: every scenario runs in a fresh child process (tests/train_child.py), one at a time, each under a time limit (tests/children.py).
The forward pass and Adam are compared to the bit; the gradient and the stats within 4 * rel_ref of the binary64 model, rel_ref being
what the same model in binary32, rows accumulated one after the other, loses against it -- the factor covers another order of the sums
and the device's exp.
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


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(tm.CASES))
def test_gradient_and_forward(case):
    """a: 85 -> 64 -> 64 at 517 rows through an index with repeats and zero weights; b: 1 -> 3, relu, 63 rows; c: 256 -> 128 x 3, 300
    rows from first_row 27 (tiles of 16 rows); d: hidden 65 (padding inside ld = 128), 257 rows; e: one-layer nets at 1 and at 64 rows.
    Each case also reads the gradient, and after an Adam step the parameters, as raw library-layout memory: the padding is zero bits."""
    assert f"gradient {case} ok" in run_child("gradient", only=case)


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
def test_the_ppo_tool_with_the_device_update():
    assert "ppo tool ok" in run_child("ppo_tool")
