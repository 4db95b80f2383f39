"""csrc/teb_fleet_host.hpp - the host rules of the _per_class calls (include/teb_amd.h: the whole tick per class): which configuration
field feeds which argument of a tick for a scene (scene_tick_params), and the feasibility specs of a fleet - the spec limits, the
range of spec_of_scene, the NULL-map rule with its count condition, the offsets of the staged footprint array, the first offending
spec and the reason - checked against hand-written answers by the stand-alone program tests/host/fleet_class_tick_host_check.cpp,
compiled with the address and undefined-behaviour sanitizers and run as a process of its own (no GPU, no HIP), as
tests/test_fleet_config_host.py does."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_fleet_class_tick_host_check(tmp_path):
    exe = os.path.join(str(tmp_path), "fleet_class_tick_host_check")
    # (the sanitizer runtimes linked statically - clang's default - so that the program does not depend on library load order)
    static = [] if "clang" in os.path.basename(CXX) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror"] + static
                          + [os.path.join(HERE, "host", "fleet_class_tick_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert "fleet class tick host check ok" in run.stdout
