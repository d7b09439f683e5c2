"""builds the stand-alone host programs of tests/host_kernels/ (the loop-restoration kernels compiled by g++ behind hip_on_host.h)"""
import os
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def build_host_program(tmp, name):
    """g++ with the sanitizers on tests/host_kernels/<name>.cpp -> the program's path"""
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "svt-av1-1_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_kernels", name + ".cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
