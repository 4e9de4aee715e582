"""The owner of every back-end handle's long-lived memory (vxu::Buf, voxel-slam_amd/csrc/vxba_buf.hpp) on the host, over a memory policy that refuses
allocations: the failure paths that no GPU test reaches without running the device out of memory."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owner_survives_every_refused_allocation(tmp_path):
    """tests/hostmath/buf_hostcheck.cpp, built with the address and undefined-behaviour sanitizers and run as a child process: one scripted life
    (reserve with growth, smaller, larger, moves onto empty and non-empty owners, a vector that reallocates, release twice, scope exit) with the k-th
    allocation refused, for every k from "never" down to the first.  After every step pointer and capacity are null / zero together, a refused growth
    leaves the owner empty and returns the error, no block is freed twice or without being live, and none is live at the end."""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "buf_hostcheck")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "hostmath", "buf_hostcheck.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    m = re.fullmatch(r"refuse never: (\d+) allocations, (\d+) frees, 0 live", lines[0])
    assert m and m.group(1) == m.group(2), lines[0]
    n = int(m.group(1))
    assert n == 15                                   # the script's allocations when none is refused: 2 + 1 + 2 + 9 + 1
    assert len(lines) == n + 1
    for k, line in zip(range(n, 0, -1), lines[1:]):
        m = re.fullmatch(rf"refuse {k}: (\d+) allocations, (\d+) frees, 0 live", line)
        assert m and int(m.group(1)) >= k and int(m.group(2)) == int(m.group(1)) - 1, line
