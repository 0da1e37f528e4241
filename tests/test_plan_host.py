"""ftgp_create's plan (the workgroup shape, the fan, the sweep's task order and task tables) compiled for the host and run without a device
(tools/plan_check.cpp) over n_rays 36 / 90 / 1080 / 1083 / 16384, 1 / 4 / 8 cars per env, small and large batches, the default fan and two
caller fans, both lidar modes, with and without FTGP_NO_PAIRS."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tools", "plan_check.cpp"), "-o", out, "-ldl", "-w"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FTGP_")}      # the plan reads FTGP_* switches: the defaults only
    r = subprocess.run([out], capture_output=True, text=True, env=env)
    return r


def test_plan_holds_what_the_step_kernel_relies_on(plan_check):
    """Each ray of each car slot drawn once in both task tables (a pair split at the tail is the one counted exception), opposite-group pairs
    exactly when the binary32 fan is point-symmetric and FTGP_NO_PAIRS is unset, whole envs of at most 16 cars per workgroup within the LDS
    cap, 8 / 16 / 64 direction sectors by car count."""
    r = plan_check
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    m = re.search(r"plan_check: (\d+) configs, (\d+) rejected, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == 540 and int(m.group(1)) - int(m.group(2)) >= 400
    assert r.stdout.count("(pairs)") > 0 and "FAIL" not in r.stdout


def test_plan_rejects_what_does_not_fit_with_todays_message(plan_check):
    out = plan_check.stdout
    assert ("rays 16384 cars_per_env 8 envs 4096 fan 0 mode 0 no_pairs 0: rejected (-1): "
            "one env of 8 car(s) with a 16384-ray scan does not fit the 160 KiB LDS") in out
    assert "rays 16385: rejected (-1): n_rays above 16384 is not supported" in out
