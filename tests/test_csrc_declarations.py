"""CPU: every host function with external linkage in csrc/ is declared in a header (csrc/host_api.h states the rule: one declaration,
in one header, included by the file that defines the function and by every file that calls it).  The compiler checks it: with
-Wmissing-prototypes it names each function defined without a previous declaration -- a hand-written prototype in a caller does not
count, the defining file never sees it.  Only `__global__` kernels may be named: a non-template kernel legitimately has no
prototype (template kernels do not warn).  Host code only, nothing is generated: -fsyntax-only with the flags of the real build."""
import glob
import importlib.util
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real_esrgan-pytorch_amd", "csrc")
_spec = importlib.util.spec_from_file_location("resr_build_for_declarations_test", os.path.join(CSRC, "build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)
HIPCC, FLAGS = _build.HIPCC, _build.FLAGS

SOURCES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
WARNING = re.compile(r"^(.+?):(\d+):\d+: warning: no previous prototype for function '([^']+)'", re.M)


def _check(name):
    return subprocess.run([HIPCC] + FLAGS + ["-Wmissing-prototypes", "--offload-host-only", "-fsyntax-only", os.path.join(CSRC, name)],
                          capture_output=True, text=True, cwd=CSRC)


@pytest.fixture(scope="module")
def diagnostics():
    """One compiler pass over every file, eight at a time, shared by the cases below."""
    if not os.path.exists(HIPCC):
        pytest.skip(f"no compiler at {HIPCC}")
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(SOURCES, ex.map(_check, SOURCES)))


def test_every_source_is_covered():
    assert len(SOURCES) >= 25 and "api.hip" in SOURCES


@pytest.mark.parametrize("name", SOURCES)
def test_only_kernels_lack_a_prototype(diagnostics, name):
    r = diagnostics[name]
    assert r.returncode == 0, r.stderr[-4000:]
    lines = {}
    undeclared = []
    for path, line, func in WARNING.findall(r.stderr):
        path = os.path.join(CSRC, path)
        if path not in lines:
            lines[path] = open(path).read().split("\n")
        if "__global__" not in lines[path][int(line) - 1]:
            undeclared.append(f"{os.path.basename(path)}:{line}: {func}")
    assert not undeclared, ("defined with external linkage and no declaration in a header (declare it in csrc/host_api.h -- conv3x3.h for "
                            "ConvArgs / ChainArgs signatures --, or make it static): " + ", ".join(sorted(set(undeclared))))
