"""csrc/teb_costmap_host.hpp - the host rules of the costmap-to-obstacles conversion that its two row kinds (points, convex polygons)
and its two routes (the single scene, a scene set) share: the lane rule, the block geometry, the filter of a pose, the layout of a set
in the shared scratch, the parse of the caller's tables and via-points, the host tables, the out-array rules - checked against
hand-written answers by the stand-alone program tests/host/costmap_host_check.cpp, compiled with the address and undefined-behaviour
sanitizers and run as a process of its own (no GPU, no HIP)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_costmap_host_check(tmp_path):
    exe = os.path.join(str(tmp_path), "costmap_host_check")
    # (the sanitizer runtimes linked statically - clang's default - so that the program does not depend on library load order)
    static = [] if "clang" in os.path.basename(CXX) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror"] + static
                          + [os.path.join(HERE, "host", "costmap_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "costmap host check ok" in run.stdout
