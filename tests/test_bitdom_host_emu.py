"""The NSGA-II fast path's kernels run on the CPU (tools_cpu/bdemu).

VERDICT r5 item 5: the m = 4 bitset dominance pass faulted on the GPU in round
4 and was deleted (commit cf1cf3a).  tools_cpu/bdemu compiles the library's
own kernel sources -- the pre-deletion tree (cf1cf3a^, kept as a snapshot in
tools_cpu/bdemu/pre_deletion) and the working tree -- as host C++ against a small HIP emulation (lanes as threads, block / wave
barriers, DPP / permlane / ballot semantics, LDS arrays poisoned before every
workgroup) and runs one whole dm_sort_nondominated call.  These tests check
that the emulated path reproduces the reference's golden order
(tests/golden/nsga2.npz, deap/tools/emo.py:53-117) for m = 2, 3 and, on the
pre-deletion tree with the bitset pass enabled for four objectives
(DM_BD_MAXM = 4), for the n = 64, M = 4 input whose first call faulted.
`tools_cpu/bdemu/run.sh` runs the same cases and synthetic 2^12 inputs under
AddressSanitizer + UBSan ("the m = 4 fault").
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EMU = os.path.join(REPO, "tools_cpu", "bdemu")


def _build(tmp, rev, name):
    out = str(tmp / "emu")
    if not os.path.exists(os.path.join(out, "cases")):
        subprocess.run(["python3", os.path.join(EMU, "make_cases.py"), os.path.join(out, "cases")],
                       check=True)
    subprocess.run(["make", "-s", "-C", EMU, "-j8", "REV=" + rev, "NAME=" + name, "SAN=0",
                    "B=" + os.path.join(out, name)], check=True, capture_output=True)
    return out


def _run(out, name, case, env=None):
    e = dict(os.environ)
    e.update(env or {})
    exe = os.path.join(out, name, "harness")
    r = subprocess.run([exe, os.path.join(out, "cases", case)], capture_output=True, text=True,
                       timeout=600, env=e)
    return r.returncode, r.stdout + r.stderr


@pytest.fixture(scope="module")
def emu_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bdemu")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("case,maxm", [("golden4.bin", "4")])
def test_pre_deletion_m4_path_on_host(emu_dir, case, maxm):
    out = _build(emu_dir, "cf1cf3a^", "pre")
    rc, log = _run(out, "pre", case, {"EMU_BD_MAXM": maxm})
    assert rc == 0, log
    assert "fronts == brute force: yes" in log
    if case.startswith("golden"):
        assert "order == reference golden: yes" in log


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("case", ["golden0.bin", "golden1.bin"])
def test_current_tree_on_host(emu_dir, case):
    out = _build(emu_dir, "worktree", "wt")
    rc, log = _run(out, "wt", case)
    assert rc == 0, log
    assert "fronts == brute force: yes" in log
    if case.startswith("golden"):
        assert "order == reference golden: yes" in log
