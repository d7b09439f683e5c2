"""The internal headers of the launch boundary under svt-av1-1_amd/csrc (no GPU needed): svthip_internal.h, one <family>_launch.h per
file prefix and pa_job_table.h each compile on their own -- a translation unit of one #include, with the Makefile's language level and
-Wall -- and nothing under csrc/ includes the me_kernels.h they replace.  So does svthip_glue.h, which the files of the C-ABI glue share:
svthip_context.hip and one <family>_abi.hip per launch header, host code that includes no other family's launch header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "svt-av1-1_amd", "csrc")
FAMILIES = ["me", "pa", "tq", "ip", "lf", "lr", "cf", "fg", "md"]
HEADERS = ["svthip_internal.h", "pa_job_table.h", "svthip_glue.h"] + [f + "_launch.h" for f in FAMILIES]


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header, tmp_path):
    assert os.path.isfile(os.path.join(CSRC, header)), header
    unit = tmp_path / "unit.hip"
    unit.write_text('#include "%s"\n' % header)
    # hipcc adds link options, which -fsyntax-only leaves unused: that driver warning is not about the header
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                        "-fsyntax-only", "-I", CSRC, str(unit)], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr and "error" not in r.stderr, r.stderr


def test_family_headers_declare_no_kernel():
    for f in FAMILIES:
        assert "__global__" not in open(os.path.join(CSRC, f + "_launch.h")).read(), f


def test_glue_is_split_by_family_and_holds_host_code_only():
    assert not os.path.exists(os.path.join(CSRC, "svthip_abi.hip"))
    for name in [f + "_abi.hip" for f in FAMILIES] + ["svthip_context.hip"]:
        assert os.path.isfile(os.path.join(CSRC, name)), name
        text = open(os.path.join(CSRC, name)).read()
        for word in ("__global__", "hipLaunchKernelGGL", "<<<", "dim3"):
            assert word not in text, (name, word)
    for f in FAMILIES:
        text = open(os.path.join(CSRC, f + "_abi.hip")).read()
        included = set(re.findall(r'#\s*include\s*["<]([a-z]+_launch\.h)[">]', text))
        # mode decision sizes the job list of the inter-prediction kernels its filter search runs (inter_pred_scratch_bytes)
        allowed = {f + "_launch.h"} | ({"ip_launch.h"} if f == "md" else set())
        assert f + "_launch.h" in included and included <= allowed, (f, sorted(included))


def test_nothing_includes_me_kernels_h():
    assert not os.path.exists(os.path.join(CSRC, "me_kernels.h"))
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r'#\s*include\s*["<][^">]*me_kernels\.h[">]', text), name
