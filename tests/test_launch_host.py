"""csrc/teb_launch_host.hpp - the host policy of the optimise launch: the layout of a handle at create, of an obstacle table and of one
launch, the helper workgroups of the multi-CU mode and their back-off, the repeat ladder after a look at the per-band flags, the
instantiation that runs - checked against hand-written answers over a synthetic LDS plan by the stand-alone program
tests/host/launch_host_check.cpp, compiled with the address and undefined-behaviour sanitizers and run as a process of its own (no GPU,
no HIP)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_launch_host_check(tmp_path):
    exe = os.path.join(str(tmp_path), "launch_host_check")
    # (the sanitizer runtimes linked statically - clang's default - so that the program does not depend on library load order)
    static = [] if "clang" in os.path.basename(CXX) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror"] + static
                          + [os.path.join(HERE, "host", "launch_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "launch host check ok" in run.stdout
