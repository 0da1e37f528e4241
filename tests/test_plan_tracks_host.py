"""ftgp_create_tracks' plan (tools/plan_tracks_check.cpp) compiled for the host and run without a device: synthetic track sets of 2 to 8
tracks, ragged env counts, 1 / 3 / 8 cars per env, 90 / 1080 rays, both lidar modes, both workgroup orders (FTGP_TRACK_ORDER)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def plan_tracks_check(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("plan_tracks") / "plan_tracks_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tools", "plan_tracks_check.cpp"), "-o", out, "-ldl", "-w"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FTGP_")}      # the plan reads FTGP_* switches: the defaults only
    return subprocess.run([out], capture_output=True, text=True, env=env, timeout=600)


def test_multi_track_plan_holds_what_the_step_kernel_relies_on(plan_tracks_check):
    """Each track's parameter block, tables and spawn table are those of a one-track plan of that track over the whole batch; every car
    sits in exactly one workgroup; a workgroup's envs share its track; each block has its own workgroups (a ragged last one); both orders
    cover the same (track, workgroup) set; the XCD order gives each track one run of residues b % 8, in track order, in proportion to
    its workgroups.  The two device images laid out from made-up addresses: every workgroup-table entry carries its track's block offset,
    the block found there has that track's size and buffers, task_tab points at the task tables behind the workgroup table, stage image k
    holds block k's head, the vehicle, track k's centre-line, the fan and both cover tables; a one-track plan's image has no table."""
    r = plan_tracks_check
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    m = re.search(r"plan_tracks_check: (\d+) configs, (\d+) rejected, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == 120 and int(m.group(2)) == 0
    assert "FAIL" not in r.stdout
