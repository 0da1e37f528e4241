"""The host side of a network slot compiled for the host and run without a device or a handle (tools/net_slot_check.cpp): every refusal of
the descriptions of a policy, its frame and rival inputs and a value net, by code and message, and for accepted descriptions over 36 / 64 /
1080 rays, 1 - 4 layers, hidden widths 1 / 63 / 64 / 65 / 128, with and without state, frame and rival inputs, every field of the record the
kernels are handed, the parameter count and the record the train kernels read.  tests/net_slot_check.txt is the output of the same cases
through the functions as they stood before the slot's host code was gathered into one struct."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def net_slot_check(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("net_slot") / "net_slot_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tools", "net_slot_check.cpp"), "-o", out, "-ldl", "-w"])
    return subprocess.run([out], capture_output=True, text=True)


def test_refusals_and_records_are_what_they_were(net_slot_check):
    r = net_slot_check
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "net_slot_check.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 500 and sum(line.startswith("refused") for line in want) > 80
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {k + 1}:\n got {g}\nwant {w}"
    assert len(got) == len(want)
