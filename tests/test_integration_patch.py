"""The reference-side integration artefacts (INTEGRATION.md Level 2): the one-word patch that makes
LinearSystemSolver::evaluateError virtual applies to the reference header, and the adapter code in INTEGRATION.md
overrides exactly the reference plugin's virtuals it forwards to the C-ABI (CPU, text checks).  The adapter's logic
itself (DV push -> device cost / build / solve, column permutation) runs in tests/test_host_cpp.py through the same
C++ host layer (TermLinearSystemSolver over the oracle-backed and the GPU solver)."""
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "patches", "aslam_backend_virtual_evaluateError.patch")
REF_HDR = "aslam_optimizer/aslam_backend/include/aslam/backend/LinearSystemSolver.hpp"


def test_patch_applies_to_reference_header():
    """The header itself is not part of this repository: tests/golden/ records its path, its length and the line of the
    declaration, and the patch carries the declaration it replaces.  The patch must apply cleanly (no offset, no fuzz)
    to a file of that shape and change that one line only."""
    if shutil.which("patch") is None:
        pytest.skip("patch(1) is not installed")
    with open(os.path.join(ROOT, "tests", "golden", "reference_linear_system_solver_hpp.json")) as f:
        rec = json.load(f)
    assert rec["header"] == REF_HDR
    removed = [l[1:] for l in open(PATCH).read().splitlines() if l.startswith("-") and not l.startswith("---")]
    assert len(removed) == 1 and "virtual" not in removed[0]
    n, at = rec["n_lines"], rec["evaluateError_declaration_line"]
    before = ["// %d" % i for i in range(1, n + 1)]
    before[at - 1] = removed[0]
    with tempfile.TemporaryDirectory() as td:
        dst = os.path.join(td, REF_HDR)
        os.makedirs(os.path.dirname(dst))
        with open(dst, "w") as f:
            f.write("\n".join(before) + "\n")
        r = subprocess.run(["patch", "-p1", "-F0", "-i", PATCH], cwd=td, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "offset" not in r.stdout and "fuzz" not in r.stdout, r.stdout
        after = open(dst).read().splitlines()
        assert len(after) == n and [i for i in range(n) if after[i] != before[i]] == [at - 1]
        assert re.search(r"virtual\s+double\s+evaluateError\(size_t nThreads, bool useMEstimator\);", after[at - 1])
        assert after[at - 1].replace("virtual ", "", 1) == before[at - 1]


def test_adapter_overrides_the_plugin_virtuals():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    adapter = doc[doc.index("class HipLinearSystemSolver"):doc.index("}}  // namespace aslam::backend")]
    for sig, call in [("void buildSystem(", "kb_build"), ("bool solveSystem(", "kb_solve"),
                      ("void setConstantConditioner(", "kb_set_constant_conditioner"),
                      ("void setConditioner(", "kb_set_conditioner"), ("double rhsJtJrhs(", "kb_rhs_jtj_rhs"),
                      ("double evaluateError(", "kb_eval_cost")]:
        i = adapter.index(sig)
        body = adapter[i:adapter.index("\n  }", i)]
        assert "override" in body.split("{")[0], sig
        assert call in body, (sig, call)
