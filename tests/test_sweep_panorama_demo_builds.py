"""The C++11 host of the composer at the swept depth -- examples/sweep_panorama_demo.cpp on tscm::Sweep::compose of
include/tscm/tscm_calib.hpp -- builds with plain g++ against libtscm_hip.so, the way tests/test_sweep_demo_builds.py builds
the depth demo, and explains itself without arguments."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_panorama_demo_compiles_and_links_against_the_abi(tmp_path):
    csrc = os.path.join(ROOT, "tscm_calib_amd", "csrc")
    exe = str(tmp_path / "a.out")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "sweep_panorama_demo.cpp"),
                           "-L", csrc, "-ltscm_hip", "-Wl,-rpath," + csrc, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
    run = subprocess.run([exe, "calib.yaml", "a.ppm", "b.ppm", "--mode", "average"], capture_output=True, text=True)
    assert run.returncode == 2 and "usage" in run.stderr
