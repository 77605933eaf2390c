"""Every SMER_* environment switch the product reads (C-ABI sources, package
Python, bench.py) is listed in DESIGN.md §9, so the runtime-switch table
stays complete as switches are added."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "smer_music_generation_amd")


def _sources():
    for d, exts in ((os.path.join(PKG, "csrc"), (".hip", ".cpp", ".h")), (PKG, (".py",))):
        for name in sorted(os.listdir(d)):
            if name.endswith(exts):
                yield os.path.join(d, name)
    yield os.path.join(ROOT, "bench.py")


def _switches():
    # getenv("SMER_X"), os.environ.get("SMER_X"), os.environ["SMER_X"], and the
    # is("SMER_X") rows of csrc/gemm.hip read_switches (one pass over environ)
    pat = re.compile(r'(?:getenv|environ\.get|environ\[|\bis)\(?\s*"(SMER_[A-Z0-9_]+)"')
    found = set()
    for path in _sources():
        with open(path) as f:
            found.update(pat.findall(f.read()))
    return found


def test_every_switch_is_documented():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    table = design[design.index("## 9. Runtime switches"):]
    switches = _switches()
    assert len(switches) > 20
    # the GEMM dispatch's own family, found through its reader
    assert {"SMER_GEMM256", "SMER_GEMM256S", "SMER_G256_NONPERSIST", "SMER_G256_SKEW", "SMER_GEMM64",
            "SMER_WGRAD256S", "SMER_SPLITK_FUSED", "SMER_GEMM_F32_MFMA", "SMER_GEMM_GLDS", "SMER_WGRAD_GLDS",
            "SMER_SPLITK_DEPTH", "SMER_WGRAD256", "SMER_WGRAD256_SLOTS", "SMER_WGRAD256_DEPTH", "SMER_SKINNY16",
            "SMER_SKINNY16_CAP", "SMER_WGRAD_WGP2", "SMER_G256_MIN", "SMER_SKINNY_KF",
            "SMER_SKINNY_ROWS_F32", "SMER_FP8_Q8_FAST", "SMER_GEMM256S_FP8"} <= switches
    missing = sorted(s for s in switches if "`%s`" % s not in table)
    assert not missing, "undocumented runtime switches: %s" % missing
