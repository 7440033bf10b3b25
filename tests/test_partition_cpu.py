"""The cut rules of csrc/token_items.h on the CPU: tests/partition_check.cpp (a stand-alone
program that includes the header alone, as plain C++17) is built with the ROCm install's host
compiler and run as a child process over its own pointer arrays and the hand-out graph
(handout_graph.py).  It asserts, under both rules, that every edge is walked by exactly the
item the rule names, every row owned by exactly one, that a row of at most `chunk` edges is
never split and no item walks more than 2 * chunk tokens under the hub rule, and that the items
reporting a continuation are exactly those whose slab the fixup reads.
"""
import os
import subprocess

import numpy as np

from handout_graph import handout_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgemm-prunning_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "partition_check.cpp")


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for p in (os.path.join(rocm, "llvm", "bin", "clang++"),
              os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(p):
            return p
    raise AssertionError(f"no clang++ under {rocm}")


def test_partition_check(tmp_path):
    exe = str(tmp_path / "partition_check")
    subprocess.check_call([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           f"-I{CSRC}", SRC, "-o", exe])
    rp = tmp_path / "handout_row_ptr.txt"
    np.savetxt(rp, handout_csr()[0], fmt="%d")
    r = subprocess.run([exe, str(rp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walks ok" in r.stdout
