"""CPU: the modules that build a reference driver through oracle/ref_driver.py -- the eight fixture generators that define build_driver and
tests/rate_util.py -- import where the reference does not exist, and say so.  That is the GPU box's situation: the *_vs_ref and *_gpu tests
import these modules there for their restatements and pictures, and the live comparisons skip on reference_available().  Each module is
imported in a fresh process, since SVT_REFERENCE_ROOT is read at import."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TESTS, GOLDEN = os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")
# module -> what its importer has on sys.path: the generators are scripts and add the rest themselves, rate_util relies on the suite's
MODULES = {**{f"make_golden_{name}": [GOLDEN] for name in ("inter_pred", "warp", "intra_pred", "cfl", "dlf", "lr", "lr_sgr", "cdef")},
           "rate_util": [TESTS, ROOT]}


@pytest.mark.parametrize("module", list(MODULES))
def test_imports_without_the_reference(module, tmp_path):
    code = (f"import sys; sys.path[:0] = {MODULES[module]!r}; import {module} as m; "
            "assert callable(m.build_reference_driver if m.__name__ == 'rate_util' else m.build_driver); "
            "assert m.reference_available() is False; print('imported')")
    env = dict(os.environ, SVT_REFERENCE_ROOT=str(tmp_path / "no_reference_here"))
    out = subprocess.run([sys.executable, "-c", code], cwd=tmp_path, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "imported", out.stderr
