"""csrc/teb_band_store.hpp and the owner of device memory under it (DevBuf, csrc/teb_scene_store.hpp) - every allocation freed exactly
once on every path, the all-or-none allocation of a set of bands, the views a BatchDev is made from, the attributes a band is born with,
the layout of the packed messages - checked against hand-written answers over counting allocation primitives by the stand-alone program
tests/host/band_store_check.cpp, compiled with the address and undefined-behaviour sanitizers and run as a process of its own (no GPU,
no HIP, leak check on)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_band_store_host_check(tmp_path):
    exe = os.path.join(str(tmp_path), "band_store_check")
    # (the sanitizer runtimes linked statically - clang's default - so that the program does not depend on library load order)
    static = [] if "clang" in os.path.basename(CXX) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror"] + static
                          + [os.path.join(HERE, "host", "band_store_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout
    assert "band store check ok" in run.stdout
