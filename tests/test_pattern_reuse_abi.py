"""CPU side of the setup keeps: the entry points and options of "pattern_reuse" / "spmv_reuse" exist, and a context that has
built nothing reports that nothing was kept."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_context(capi):
    return capi.Context(device=-1)


def test_header_and_bindings_declare_the_info_calls(fedd_lib):
    txt = open(os.path.join(ROOT, "include", "fedd_hip.h")).read()
    for name in ("fedd_pattern_reuse_info", "fedd_spmv_reuse_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/fedd_hip.h"
        assert name in fedd_lib.SIGNATURES
        assert hasattr(fedd_lib.lib(), name)
    for opt in ('"pattern_reuse"', '"spmv_reuse"'):
        assert opt in txt, "option %s is not described in include/fedd_hip.h" % opt


def test_options_exist_and_nothing_was_kept_yet(fedd_lib):
    c = _host_context(fedd_lib)
    try:
        for opt in ("pattern_reuse", "spmv_reuse"):
            c.set_option(opt, 0)
            c.set_option(opt, 1)
        assert c.pattern_reuse_info() == {"last_reused": False, "n_reused": 0}
        assert c.spmv_reuse_info() == {"last_reused": False, "n_reused": 0}
    finally:
        c.close()
