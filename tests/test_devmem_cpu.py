"""The handle's memory-ownership rule (csrc/mds_devmem.hpp) without a GPU: the header compiled with g++ under AddressSanitizer + UBSan
against an allocator that fails on request (tests/devmem_main.cpp), run as a program of its own."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ownership_rule_under_a_failing_allocator(tmp_path):
    """Groups of 1 to 5 fields with every allocation and every zero-fill failing in turn, with and without a field allocated beforehand:
    all-or-nothing, nothing leaked; zero-filled fields read zero; replace keeps the old block until the new one is complete; release and
    release_all any number of times in any order.  ASan (leaks, double frees) and UBSan end the program with a non-zero status."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the ownership rule's stand-alone program"
    exe = str(tmp_path / "devmem_main")
    # the sanitizer runtimes linked statically: the program needs nothing preloaded and is indifferent to what the environment preloads
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "devmem_main.cpp")])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stdout[-2000:], done.stderr[-2000:])
    assert done.stdout.strip() == "ok"
