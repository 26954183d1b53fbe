"""Building and running the CPU checks of the host plan headers (tests/native/*.cpp against tscm_calib_amd/csrc/*.h):
what every test module of a header shares.  A check is one g++ translation unit that prints one JSON line.  No GPU."""
import functools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CXX = ["g++", "-std=c++17", "-Wall", "-Werror"]
NEEDS_GXX = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
SANITIZE = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(src, name, flags):
    """tests/native/<src> -> tmp/<name>; returns the path and the compiler's result."""
    exe = os.path.join(ROOT, "tmp", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    r = subprocess.run([*CXX, *flags, "-o", exe, os.path.join(NATIVE, src)], capture_output=True, text=True)
    return exe, r


@functools.lru_cache(maxsize=None)
def built(src, name):
    """The plain build of a check, once per process (for helpers that tests call outside a fixture)."""
    exe, r = build(src, name, ["-O2"])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def checker_fixture(src, stem, include=None):
    """The module's `checker` fixture: the check built plain, and under AddressSanitizer + UBSan.  include: one more include
    path, relative to the repository (for a check of a header under include/)."""
    extra = ["-I", os.path.join(ROOT, include)] if include else []

    @pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
    def checker(request):
        if request.param == "plain":
            exe, r = build(src, stem, ["-O2", *extra])
        else:
            exe, r = build(src, stem + "_san", [*SANITIZE, *extra])
            if r.returncode != 0 and "asan" in (r.stderr + r.stdout).lower():
                pytest.skip("sanitizer runtime not installed")
        assert r.returncode == 0, r.stderr[-2000:]
        return exe
    return checker


def run(exe, *args, stdin=None):
    r = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout)


def assert_plain_cpp17(header):
    r = subprocess.run([*CXX, "-fsyntax-only", os.path.join(ROOT, "tscm_calib_amd", "csrc", header)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
