"""kb_set_robust_build on the CPU: the layout decision in kalibr_amd/csrc/kb_build_layout.h (robust_pipe / robust_fits,
compiled on the host as tests/test_build_layout.py does) and the declaration in include/kalibr_hip.h.

The rig is tests/test_build_layout.py's: N = 8, C = 106, K = 512.  k_build needs 18836 + 1536 + 8 ceil(F / 512) doubles
of LDS against 20480, so it fits up to F = 6656; k_buildp drops the staged target when there is no room and takes the
rig far beyond.  A weighted handle in KB_ROBUST_BUILD_GENERAL mode builds with k_build and is refused from F = 6657 on;
in KB_ROBUST_BUILD_PIPE mode it keeps kb_create's k_buildp layout and is accepted."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4 = dict(N=8, C=106, wpb=8, bpc=1)


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("robust_build_layout") / "test_robust_build_layout")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", out,
                    os.path.join(ROOT, "tests", "cpp", "test_robust_build_layout.cpp")], check=True)

    def run(N, C, K, wpb, bpc, F, pipe0=True):
        r = subprocess.run([out, *map(str, (N, C, K, wpb, bpc, F, int(pipe0)))], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stderr
        v = [bool(int(x)) for x in r.stdout.split()]
        keys = [("general", False), ("general", True), ("pipe", False), ("pipe", True)]
        return {k: dict(pipe=v[2 * i], fits=v[2 * i + 1]) for i, k in enumerate(keys)}

    return run


def test_general_refuses_what_pipe_accepts(decide):
    assert 18836 + 1536 + 8 * 13 <= 160 * 1024 // 8 < 18836 + 1536 + 8 * 14  # k_build: 13 frames per block at most
    over = decide(K=512, F=6657, **C4)
    assert not over[("general", True)]["fits"] and not over[("general", True)]["pipe"]
    assert over[("pipe", True)]["fits"] and over[("pipe", True)]["pipe"]
    at = decide(K=512, F=6656, **C4)
    assert at[("general", True)]["fits"] and at[("pipe", True)]["fits"]


def test_an_unweighted_handle_is_kb_creates_in_both_modes(decide):
    for F in (6656, 6657, 2000):
        r = decide(K=512, F=F, **C4)
        assert r[("general", False)] == r[("pipe", False)] == dict(pipe=True, fits=True)


def test_a_k_build_rig_stays_on_k_build(decide):
    # two cameras (kb_create chose k_build: pipe0 = 0): the mode cannot bring k_buildp
    r = decide(N=2, C=22, K=144, wpb=4, bpc=2, F=12, pipe0=False)
    assert all(not v["pipe"] and v["fits"] for v in r.values())


def test_the_header_declares_it_and_the_library_defines_it():
    hdr = open(os.path.join(ROOT, "include", "kalibr_hip.h")).read()
    m = re.search(r"enum\s+kb_robust_build\s*\{([^}]*)\}", hdr)
    assert m, "enum kb_robust_build"
    vals = dict((k.strip(), int(v)) for k, v in (x.split("=") for x in m.group(1).split(",")))
    assert vals == {"KB_ROBUST_BUILD_GENERAL": 0, "KB_ROBUST_BUILD_PIPE": 1}
    assert re.search(r"\bint\s+kb_set_robust_build\s*\(\s*kb_handle\s*\*\s*h\s*,\s*int32_t\s+mode\s*\)\s*;", hdr)
    src = open(os.path.join(ROOT, "kalibr_amd", "csrc", "kb_capi.hip")).read()
    assert re.search(r"^int kb_set_robust_build\(kb_handle\* h, int32_t mode\) \{", src, re.M)
    from kalibr_amd import capi
    assert "kb_set_robust_build" in capi.EXPORTS and capi.ROBUST_BUILDS == {"general": 0, "pipe": 1}


def test_the_mode_setter_asks_before_it_changes_a_weighted_handle():
    src = open(os.path.join(ROOT, "kalibr_amd", "csrc", "kb_capi.hip")).read()
    f = src[src.index("int kb_set_robust_build("):]
    f = f[:f.index("\n}\n")]
    assert 0 < f.index("robust_fits(h, true, mode)") < f.index("h->rb_build = mode;\n  h->sys_valid")
    assert f.index("build_pipe0") < f.index("h->rb_build = mode;") and f.index("sharded(h)") < f.index("h->rb_build = mode;")
