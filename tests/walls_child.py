"""Child process of tests/test_walls_model.py: one GPU scenario per process.  Exit status 0 = the scenario held.

    python tests/walls_child.py rays <scene>
    python tests/walls_child.py contacts <scene>

`rays`: the binary64 wall-ray model's assertions on libftgp.so, and libftgp.so = the oracle's plain specification bit for bit on the same
scan.  `contacts`: the binary64 wall-contact model's assertions on libftgp.so; then libftgp.so = oracle bit for bit after that step and
after 200 more under the random policy, as `contacts` of tests/crowded_child.py does.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

os.environ["FTGP_VERBOSE"] = "1"          # ftgp_create's lines about the workgroup shape go to stderr and into the test's report

from tests import walls_model as T  # noqa: E402
from tests.helpers import libs, same  # noqa: E402


def rays(name):
    product, oracle = libs()
    T.check_rays(product, name)
    sc = T.RAY_SCENES[name]()
    _, got = T.scan(product, sc)
    _, spec = T.scan(oracle, sc, mode=2)
    np.testing.assert_array_equal(got, spec, err_msg=f"{name}: libftgp.so against the oracle's plain specification")
    print("rays ok")


def contacts(name):
    product, oracle = libs()
    T.check_contacts(product, name)
    sc = T.contact_scene(name)
    multi = len(sc.tracks) > 1
    n_block = len(sc.pos) // len(sc.tracks)
    g = T.contact_env(product, sc, sc.tracks, seed=9)
    # the oracle takes one track per handle: a multi-track handle is compared block by block (env_base = the block's first env)
    os_ = [T.contact_env(oracle, block(sc, k, n_block) if multi else sc, [t], seed=9, env_base=k * n_block // sc.cpe) for k, t in enumerate(sc.tracks)]
    with g:
        for k, o in enumerate(os_):
            oracle.dll.oracle_set_threads(o.h, 8)
            T.prepare(o, block(sc, k, n_block) if multi else sc)
        T.prepare(g, sc)
        for e in [g] + os_:
            e.step(1)
        if not multi:
            same(g, os_[0], f"{name}: one step")
            for e in (g, os_[0]):
                e.rollout("random", 200)
            same(g, os_[0], f"{name}: 200 steps of the random policy after it")
        else:
            for steps in (0, 200):
                if steps:
                    for e in [g] + os_:
                        e.rollout("random", steps)
                for k, o in enumerate(os_):
                    rows = slice(k * n_block, (k + 1) * n_block)
                    np.testing.assert_array_equal(g.pose()[rows], o.pose(), err_msg=f"{name}: block {k} after {steps} more steps: pose")
                    np.testing.assert_array_equal(g.lidar()[rows], o.lidar(), err_msg=f"{name}: block {k} after {steps} more steps: lidar")
        for o in os_:
            o.close()
    print("contacts ok")


def block(sc, k, n):
    import dataclasses
    rows = slice(k * n, (k + 1) * n)
    return dataclasses.replace(sc, tracks=[sc.tracks[k]], pos=sc.pos[rows], yaw=sc.yaw[rows], vel=sc.vel[rows])


if __name__ == "__main__":
    {"rays": rays, "contacts": contacts}[sys.argv[1]](sys.argv[2])
