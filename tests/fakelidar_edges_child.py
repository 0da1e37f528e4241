"""Child process of tests/test_fakelidar_mode.py: one GPU scenario per process, torch imported before libftgp.so is loaded (see
ft_grandprix_amd/vec.py).  Exit status 0 = the scenario held; anything else fails the test that started it.

    python tests/fakelidar_edges_child.py <scenario> [json options]

All comparisons are bit for bit.  The fixture is G10 (tests/golden/make_golden.py: gen_g10), the reference's raycast.fakelidar at the
image's edges; the checks are those the oracle passes on the CPU (tests/helpers.py).
`edges`: one ftgp_step from the G10 poses on every G10 image at R = 72 and 37 -- opt: cars_per_env (1: 64 envs; 3: 22 envs, the MULTI
kernel), cars_per_block (FTGP_CARS_PER_BLOCK; one that does not divide the car count gives a ragged last workgroup).
`edges_tracks`: the 61 x 127 and the 200 x 333 image in one ftgp_create_tracks handle, 40 + 24 envs; each track's distance transform.
`edt`: ftgp_edt_kernel against scipy.ndimage.distance_transform_edt as arrays: ragged shapes, one wall pixel, wall-free columns, runs of 2000.
`loop`: closed loops from poses on and off the 200 x 333 image, GPU against oracle -- opt: config (an index into helpers.G10_LOOPS).
`standalone`: ftgp_fakelidar on the L-wall images and the single rays of G10.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library is loaded)
import numpy as np  # noqa: E402

from ft_grandprix_amd import capi  # noqa: E402
from tests import helpers as hp  # noqa: E402

def edges(opt):
    lib, _ = hp.libs()
    os.environ["FTGP_VERBOSE"] = "1"                              # ftgp_create reads both: set before the handles exist
    if opt.get("cars_per_block") is not None:
        os.environ["FTGP_CARS_PER_BLOCK"] = str(int(opt["cars_per_block"]))
    hp.check_g10_steps(lib, hp.g10(), cars_per_env=int(opt.get("cars_per_env", 1)))
    print("edges ok")


def edges_tracks(opt):
    from scipy.ndimage import distance_transform_edt
    lib, _ = hp.libs()
    g = hp.g10()
    keys, counts = ("img3", "img4"), (40, 24)
    tracks = [hp.g10_track(g, k) for k in keys]
    idx = (np.arange(40), 20 + np.arange(24))                   # both blocks hold poses on and off their image
    xy = np.concatenate([g[f"{k}_xy"][i] for k, i in zip(keys, idx)])
    quat = np.concatenate([g[f"{k}_quat"][i] for k, i in zip(keys, idx)])
    for R in hp.G10_RAYS:
        got = hp.fakelidar_step(lib, tracks, xy, quat, R, None, envs_per_track=counts)
        want = np.concatenate([g[f"{k}_{R}_ranges"][i] for k, i in zip(keys, idx)])
        np.testing.assert_array_equal(got, want, err_msg=f"two tracks, R = {R}")
    with capi.Env(lib, tracks, n_envs=64, n_rays=8, lidar_mode="fakelidar", envs_per_track=counts) as e:
        for k, t in enumerate(tracks):
            np.testing.assert_array_equal(e.get_distance_field(k), distance_transform_edt(~t.wall_mask()), err_msg=f"distance transform of track {k}")
    print("edges_tracks ok")


def edt(opt):
    from scipy.ndimage import distance_transform_edt
    lib, _ = hp.libs()
    g = hp.g10()
    walls = hp.odd_walls()                                       # the images the oracle's transform is checked on
    walls += [hp.g10_track(g, f"img{k}").wall_mask() for k in range(5)] + [hp.g10_track(g, f"L{k}").wall_mask() for k in range(2)]
    for (H, W), (y, x) in (((3, 2000), (2, 1999)), ((2000, 3), (0, 2)), ((3, 2000), (0, 0)), ((2000, 3), (1999, 0))):
        wall = np.zeros((H, W), dtype=bool)                      # one wall pixel in a corner: wall-free columns, walks and runs of 2000
        wall[y, x] = True
        walls.append(wall)
    for wall in walls:
        H, W = wall.shape
        with capi.Env(lib, hp.image_track(hp.pack_walls(wall), H, W), n_envs=1, n_rays=8, lidar_mode="fakelidar") as e:
            dt = e.distance_field()
        np.testing.assert_array_equal(dt, distance_transform_edt(~wall), err_msg=f"{H} x {W}, {int(wall.sum())} wall pixels")
    print(f"edt ok: {len(walls)} images")


def loop(opt):
    lib, ora = hp.libs()
    cars, policy, R = hp.G10_LOOPS[int(opt["config"])]
    t = hp.g10_track(hp.g10(), "img4")
    kw = dict(n_envs=24, cars_per_env=cars, n_rays=R, spawn_mode=1, seed=11, lidar_mode="fakelidar")
    with capi.Env(lib, t, **kw) as g, capi.Env(ora, t, **kw) as o:
        ora.dll.oracle_set_threads(o.h, 8)
        hp.g10_closed_loop(g, o, policy)
        assert g.kernel_name() == f"ftgp_step_kernel<{'true' if cars > 1 else 'false'}, true, true>", g.kernel_name()      # <MULTI, FAKE, ROSTER>
    print("loop ok")


def standalone(opt):
    lib, _ = hp.libs()
    hp.check_g10_standalone(lib, hp.g10())
    print("standalone ok")


SCENARIOS = {"edges": edges, "edges_tracks": edges_tracks, "edt": edt, "loop": loop, "standalone": standalone}

if __name__ == "__main__":
    t0 = time.perf_counter()
    SCENARIOS[sys.argv[1]](json.loads(sys.argv[2]) if len(sys.argv) > 2 else {})
    print(f"{sys.argv[1]}: {time.perf_counter() - t0:.2f} s")
