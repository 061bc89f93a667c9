"""The receive path's host decisions on the CPU (csrc/qpsk_rx_plan.h): which
rx_kernel instantiation a batch gets (thresholds of DESIGN.md "Kernels" on a
256-CU device, forced shape, width and priority), the layout of the
host-memory entry point's staging block, the alignment rule of a receive call's
device pointers, and the snapshot size.  The header
makes no HIP runtime call, so tests/sanitize/rx_plan_check.cc is built with
plain g++ under ASan + UBSan and run here; any report or failed check fails
the test.  CPU only."""
import pytest

from plan_check import plan_limits, run_plan_check


@pytest.fixture(scope="module")
def plan_out(tmp_path_factory):
    return run_plan_check(tmp_path_factory.mktemp("plan"))


def test_shapes_and_staging_layout(plan_out):
    """Every check of the stand-alone program held (it prints the ones that
    did not and exits nonzero) and it ran to its end."""
    assert "FAILED" not in plan_out
    assert plan_out.count("state_size") == 5


def test_state_size_matches_the_abi_formula(plan_out):
    """rx_state_size, which qpsk_rx_state_size returns, against the formula of
    tests/test_abi.py::test_state_snapshot_size."""
    per = 2 * 1880 * 2 + 168 * 8 + 4 + 4
    got = {int(l.split()[1]): int(l.split()[2]) for l in plan_out.splitlines() if l.startswith("state_size")}
    assert got == {0: 0, -3: 0, 1: 64 + per, 96: 64 + 96 * per, 65536: 64 + 65536 * per}


def test_pointer_rule_and_staging_views(plan_out):
    """rx_ptrs_aligned at every offset 0..15 of each pointer and with the
    optional ones NULL, and the views of stage_of(cf) for cf = 1..70 and around
    the pinned limit (pointers() of the program: a failed check prints FAILED
    with its line).  The limits it prints are the ones the host-call cases of
    tests/test_gpu_rx_writeset.py sit at."""
    assert "FAILED" not in plan_out
    zero_copy, pinned = plan_limits(plan_out)
    assert zero_copy == 64
    # 3760 bytes of input per channel-frame, rounded up to 256, within 8 MiB
    assert -(-3760 * pinned // 256) * 256 <= 8 << 20 < -(-3760 * (pinned + 1) // 256) * 256
