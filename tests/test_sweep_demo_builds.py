"""The C++11 host of the sphere sweep -- examples/sweep_depth_demo.cpp on the classes of include/tscm/tscm_calib.hpp -- builds
with plain g++ against libtscm_hip.so, the way tests/test_abi.py builds the other hosts, and explains itself without arguments."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_depth_demo_compiles_and_links_against_the_abi(tmp_path):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "a.out")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sweep_depth_demo.cpp"),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
