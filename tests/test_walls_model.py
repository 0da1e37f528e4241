"""The wall half of the world -- rangefinder rays against wall pixels (K2), wall contact forces (K1 step 4) -- against the binary64
models of tests/walls_model.py (their derivation, tolerances and what was measured: that module's docstring).  The check functions
run on the oracle here and on libftgp.so under `-m gpu`, one scenario per fresh child process (tests/walls_child.py).
"""
import dataclasses
import functools
import os

import numpy as np
import pytest

from ft_grandprix_amd.track import load_track
from tests import children
from tests.helpers import check, k2_minus_fakelidar_square_pixels
from tests.walls_model import CONTACT_SCENES, GPU_ONLY_CONTACT_SCENES, RAY_SCENES, check_contacts, check_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "walls_child.py")


# ============================================================================================================ on the CPU
# every scene on the oracle's default march; its plain specification (lidar_mode 2) on one scene of each kind
ORACLE_RAY_CASES = [(n, 0) for n in RAY_SCENES] + [(n, 2) for n in ("bundled-track", "needles", "strip", "mates")]


@pytest.mark.parametrize("name,mode", ORACLE_RAY_CASES, ids=[f"{n}-{'plain-spec' if m else 'march'}" for n, m in ORACLE_RAY_CASES])
def test_oracle_wall_rays_meet_the_binary64_model(oracle, name, mode):
    check_rays(oracle, name, mode)


@pytest.mark.parametrize("name", list(CONTACT_SCENES))
def test_oracle_wall_contacts_meet_the_binary64_model(oracle, name):
    check_contacts(oracle, name)


def wrong_tracks(t):
    """The track wrong in one way each."""
    return {"origin_x half a pixel off": dataclasses.replace(t, origin_x=t.origin_x + 0.5 * t.px_size_x),
            "bitmap rolled by one row": dataclasses.replace(t, bits=np.roll(t.bits, 1, axis=0)),
            "px_size_x and px_size_y exchanged": dataclasses.replace(t, px_size_x=t.px_size_y, px_size_y=t.px_size_x),
            "y mirrored": dataclasses.replace(t, bits=np.ascontiguousarray(t.bits[::-1]))}


@pytest.mark.parametrize("wrong", ["origin_x half a pixel off", "bitmap rolled by one row", "px_size_x and px_size_y exchanged", "y mirrored"])
def test_the_ray_model_is_sensitive_to_the_wall_frame(oracle, wrong):
    """The library is handed a Track that is wrong in one way while the model keeps the true one (`inkscape`, a 2133-pixel track: its pixels
    are not square in the wall frame): the model's assertions fail, every time.

    What tests/test_k2_reference_pin.py makes of the first two (its `check`, the library told the wrong track, the cars posed in the true
    one; measured on the oracle, all four tracks, 36 and 1080 rays).  Its median ([0, 2.5] px) and its share inside [-1.5, 4] px (85 %) see
    neither: median 0.79 .. 1.18, share 0.837 .. 0.959 with the wrong frames against 0.84 .. 1.22 and 0.888 .. 0.963 with the true one.  Its
    every-ray bound (>= -1.5 px; -1.07 .. -1.36 with the true frame) is all that notices: half a pixel reads -1.32 .. -1.71 -- it passes
    with the 36-ray goldens of `inkscape`, asserted here -- and one row -1.71 .. -2.23, caught by a fifth to three quarters of a pixel,
    where the model below misses its tolerance by four orders of magnitude."""
    name = "inkscape"
    t = load_track(name)
    assert t.px_size_x != t.px_size_y
    with pytest.raises(AssertionError):
        check_rays(oracle, f"bundled-{name}", lib_track=wrong_tracks(t)[wrong])
    if wrong == "origin_x half a pixel off":
        check(k2_minus_fakelidar_square_pixels(oracle, name, 36, wrong=lambda sq: wrong_tracks(sq)[wrong]))
    if wrong == "bitmap rolled by one row":
        for R in (36, 1080):
            d = k2_minus_fakelidar_square_pixels(oracle, name, R, wrong=lambda sq: wrong_tracks(sq)[wrong])
            print(f"one row, {R} rays: min {d.min():.2f}, median {np.median(d):.2f}, inside {((d >= -1.5) & (d <= 4.0)).mean():.3f}")
            assert 0.0 <= np.median(d) <= 2.5 and ((d >= -1.5) & (d <= 4.0)).mean() >= 0.85          # two of the pin's three criteria pass
            with pytest.raises(AssertionError):                                                          # its every-ray bound does not
                check(d)


def test_the_contact_model_is_sensitive_to_damping_and_torque_arm(oracle):
    """The library is handed a vehicle with another damping, or with a circle elsewhere on the axis, while the model keeps the true one:
    the contact assertions fail."""
    for tamper in (lambda v: setattr(v, "contact_damping", 0.99 * v.contact_damping), lambda v: v.contact_x.__setitem__(0, 0.99 * v.contact_x[0])):
        with pytest.raises(AssertionError):
            check_contacts(oracle, "leaning", tamper)


# ============================================================================================================ on the GPU
run_child = functools.partial(children.run_child, CHILD, timeout=300)          # this module's child script and time limit


# the smallest scene first; the 8192-pixel strip, the largest image the library accepts, last
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["needles-37"] + [n for n in RAY_SCENES if n not in ("needles-37", "strip")])
def test_gpu_wall_rays_meet_the_binary64_model(name):
    run_child("rays", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTACT_SCENES) + list(GPU_ONLY_CONTACT_SCENES))
def test_gpu_wall_contacts_meet_the_binary64_model(name):
    run_child("contacts", name)


@pytest.mark.gpu
def test_gpu_wall_rays_on_the_largest_image_meet_the_binary64_model():
    run_child("rays", "strip")
