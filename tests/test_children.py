"""The runner of the suite's child processes (tests/children.py) on a stub child: a few lines of Python that write a marker file, print
a text and leave with a status, or sleep past the time limit.  No GPU, no signals; every test passes its own `crashed` list, so the
session's list is never touched.
"""
import os

import pytest

from tests.children import CRASHED, GPU_FAULTS, run_child

STUB = """import os, sys, time
open(os.path.join(os.path.dirname(os.path.abspath(__file__)), sys.argv[1] + ".started"), "w").close()
print(sys.argv[3], file=sys.stderr if sys.argv[1] == "stderr" else sys.stdout)
if sys.argv[1] == "sleep":
    time.sleep(30)
sys.exit(int(sys.argv[2]))
"""


@pytest.fixture
def stub(tmp_path):
    """The stub's path: `python stub_child.py <scenario> <status> <text>` writes `<scenario>.started` beside itself."""
    path = tmp_path / "stub_child.py"
    path.write_text(STUB)
    return str(path)


def started(stub, scenario):
    return os.path.exists(os.path.join(os.path.dirname(stub), scenario + ".started"))


def test_status_0_returns_stdout_and_stderr(stub):
    crashed = []
    assert "hello" in run_child(stub, "ok", "0", "hello", timeout=10, crashed=crashed)
    assert "from stderr" in run_child(stub, "stderr", "0", "from stderr", timeout=10, crashed=crashed)
    assert crashed == [] and started(stub, "ok")


def test_the_command_line_is_scenario_arguments_and_options(stub):
    """A bare argument stays bare (tests/walls_child.py); options go as one JSON object, an empty one too when there are no arguments."""
    echo = os.path.join(os.path.dirname(stub), "echo_child.py")
    with open(echo, "w") as f:
        f.write("import sys\nprint(sys.argv[1:])\n")
    assert "['rays', 'needles-37']\n" in run_child(echo, "rays", "needles-37", timeout=10, crashed=[])
    assert "['errors', '{}']\n" in run_child(echo, "errors", timeout=10, crashed=[])
    assert """['twin', '{"calls": 200, "roster": ["agent", "nidc"]}']\n""" in run_child(echo, "twin", timeout=10, crashed=[], calls=200, roster=["agent", "nidc"])


def test_status_1_fails_its_test_and_stops_nothing(stub):
    crashed = []
    with pytest.raises(AssertionError, match="exit status 1"):
        run_child(stub, "plain", "1", "an assertion of the scenario failed", timeout=10, crashed=crashed)
    assert crashed == []
    assert "next" in run_child(stub, "after", "0", "next", timeout=10, crashed=crashed)


@pytest.mark.parametrize("status", [134, 139])
def test_abort_and_segmentation_fault_statuses_fill_the_list(stub, status):
    crashed = []
    with pytest.raises(AssertionError, match=f"exit status {status}"):
        run_child(stub, "died", str(status), "x", timeout=10, crashed=crashed)
    assert len(crashed) == 1 and "stub_child.py died" in crashed[0] and f"exit status {status}" in crashed[0]


def test_the_time_limit_fills_the_list(stub):
    crashed = []
    with pytest.raises(AssertionError, match="no end after 1 s"):
        run_child(stub, "sleep", "0", "x", timeout=1, crashed=crashed)
    assert len(crashed) == 1 and "no end after 1 s" in crashed[0] and started(stub, "sleep")


@pytest.mark.parametrize("status", [1, 0])
def test_a_gpu_fault_in_the_output_fills_the_list_whatever_the_status(stub, status):
    crashed = []
    text = "RuntimeError: HIP error: an illegal memory access was encountered"
    assert GPU_FAULTS[0] in text
    with pytest.raises(AssertionError, match="illegal memory access"):
        run_child(stub, "stderr", str(status), text, timeout=10, crashed=crashed)
    assert len(crashed) == 1 and GPU_FAULTS[0] in crashed[0]


def test_a_filled_list_refuses_the_next_child_without_starting_it(stub):
    crashed = []
    with pytest.raises(AssertionError):
        run_child(stub, "died", "139", "x", timeout=10, crashed=crashed)
    with pytest.raises(AssertionError, match=r"not started: an earlier GPU scenario died \(stub_child.py died 139 x: exit status 139\)"):
        run_child(stub, "next", "0", "never", timeout=10, crashed=crashed)
    assert started(stub, "died") and not started(stub, "next") and len(crashed) == 1


def test_the_sessions_list_is_the_default():
    assert run_child.__kwdefaults__["crashed"] is CRASHED
