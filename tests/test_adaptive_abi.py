"""Adaptive sampling's C ABI without a device: the entry points are exported, the header is still C99, the ctypes layout of
SolAdaptive matches the C compiler's, and configuration errors are refused before any device call."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import parity_util  # noqa: F401  (puts the package on sys.path)
from solstrale_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["sol_adaptive_begin", "sol_adaptive_round", "sol_adaptive_counts", "sol_tonemap_rgb8_adaptive", "sol_adaptive_rescale"]


def test_entry_points_are_exported():
    lib = _abi.load_hip()
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert n in _abi.HIP_SYMBOLS
    assert hasattr(_abi.load_host(), "solh_set_adaptive")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_is_c99_and_layout_matches(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "solstrale_hip.h"
#include "solstrale_host.h"
int main(void) {
  printf("%u %u %u %u %u %u\\n", (unsigned)sizeof(SolAdaptive), (unsigned)offsetof(SolAdaptive, size), (unsigned)offsetof(SolAdaptive, round),
         (unsigned)offsetof(SolAdaptive, min_samples), (unsigned)offsetof(SolAdaptive, max_samples), (unsigned)offsetof(SolAdaptive, threshold));
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.SolAdaptive
    assert got == [C.sizeof(S), S.size.offset, S.round.offset, S.min_samples.offset, S.max_samples.offset, S.threshold.offset]


def _begin(lib, **kw):
    cfg = dict(size=C.sizeof(_abi.SolAdaptive), round=16, min_samples=32, max_samples=64, threshold=0.05)
    cfg.update(kw)
    return lib.sol_adaptive_begin(None, C.byref(_abi.SolAdaptive(**cfg)))


@pytest.mark.parametrize("bad", [dict(round=0), dict(round=8), dict(round=24), dict(min_samples=24), dict(min_samples=80),
                                 dict(max_samples=0, min_samples=0), dict(threshold=-0.1), dict(threshold=float("nan")), dict(size=8)],
                         ids=["round0", "round8", "round24", "min24", "min_gt_max", "max0", "negative", "nan", "size"])
def test_configuration_errors_need_no_device(bad):
    lib = _abi.load_hip()
    assert _begin(lib, **bad) == _abi.SOL_EINVAL
    assert b"sol_adaptive_begin" in lib.sol_last_error()  # refused for the configuration, not for the missing scene


def test_valid_configuration_reaches_the_scene_check():
    lib = _abi.load_hip()
    assert _begin(lib) == _abi.SOL_EINVAL
    assert lib.sol_last_error() == b"null scene"
    assert lib.sol_adaptive_begin(None, None) == _abi.SOL_EINVAL
    n = C.c_uint32()
    assert lib.sol_adaptive_round(None, 1, C.byref(n)) == _abi.SOL_EINVAL
    assert lib.sol_adaptive_counts(None, None, 0) == _abi.SOL_EINVAL
    assert lib.sol_tonemap_rgb8_adaptive(None, None, None) == _abi.SOL_EINVAL
    assert lib.sol_adaptive_rescale(None, None) == _abi.SOL_EINVAL


def test_host_setting_is_validated():
    lib = _abi.load_host()
    b = lib.solh_builder_new()
    try:
        assert lib.solh_set_adaptive(b, 16, 32, 0.05) == 0
        assert lib.solh_set_adaptive(b, 0, 0, 0.0) == 0  # off
        for args in ((8, 32, 0.05), (16, 20, 0.05), (16, 32, -1.0), (16, 32, float("nan"))):
            assert lib.solh_set_adaptive(b, *args) < 0, args
    finally:
        lib.solh_builder_free(b)
